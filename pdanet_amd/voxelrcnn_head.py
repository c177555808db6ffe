"""VoxelRCNNHead (pcdet/models/roi_heads/voxelrcnn_head.py): RoI-grid pooling over the 3D backbone's sparse levels
(voxel_pool_modules.NeighborVoxelSAModuleMSG, fused in csrc/voxel_pool.hip), three fc stacks, the rcnn losses of
RoIHeadTemplate -- under the reference's module names, so a reference checkpoint loads with strict=True.

The grid-point arithmetic is the reference's torch expressions (its float `//` included).  Where the reference fills the
per-scene voxel counts and the batch column in Python loops, this compares against an arange: the counts stay on the device
and the training path reads nothing on the host.  The model config is not modified (the reference prepends the input
channels to ROI_GRID_POOL.POOL_LAYERS.*.MLPS in place).

Target sampling: batch_dict may carry 'roi_target_seed' or 'roi_target_draws' (ProposalTargetLayer.forward's seed / draws).

Out of scope: GRID_3D_IOU_LOSS, graph capture of the head."""
import torch
import torch.nn as nn

from .roi_head_template import RoIHeadTemplate
from .voxel_pool_modules import NeighborVoxelSAModuleMSG
from .voxel_utils import generate_voxel2pinds, get_voxel_centers


class VoxelRCNNHead(RoIHeadTemplate):
    def __init__(self, backbone_channels, model_cfg, point_cloud_range, voxel_size, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.pool_cfg = model_cfg['ROI_GRID_POOL']
        if model_cfg['LOSS_CONFIG'].get('GRID_3D_IOU_LOSS', False):
            raise NotImplementedError("GRID_3D_IOU_LOSS")
        layer_cfg = self.pool_cfg['POOL_LAYERS']
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.voxel_size = [float(v) for v in voxel_size]

        c_out = 0
        self.roi_grid_pool_layers = nn.ModuleList()
        for src_name in self.pool_cfg['FEATURES_SOURCE']:
            cfg = layer_cfg[src_name]
            mlps = [[backbone_channels[src_name]] + list(m) for m in cfg['MLPS']]
            self.roi_grid_pool_layers.append(NeighborVoxelSAModuleMSG(
                query_ranges=cfg['QUERY_RANGES'], nsamples=cfg['NSAMPLE'], radii=cfg['POOL_RADIUS'], mlps=mlps,
                pool_method=cfg['POOL_METHOD']))
            c_out += sum(x[-1] for x in mlps)

        grid = self.pool_cfg['GRID_SIZE']
        pre_channel = grid * grid * grid * c_out
        dp = model_cfg['DP_RATIO']

        def fc_stack(widths, pre, inplace):
            layers = []
            for k, width in enumerate(widths):
                layers.extend([nn.Linear(pre, width, bias=False), nn.BatchNorm1d(width), nn.ReLU(inplace=inplace)])
                pre = width
                if k != len(widths) - 1 and dp > 0:
                    layers.append(nn.Dropout(dp))
            return nn.Sequential(*layers), pre

        self.shared_fc_layer, pre_channel = fc_stack(model_cfg['SHARED_FC'], pre_channel, True)
        self.cls_fc_layers, cls_channel = fc_stack(model_cfg['CLS_FC'], pre_channel, False)
        self.cls_pred_layer = nn.Linear(cls_channel, self.num_class, bias=True)
        # the reference chains pre_channel through the cls stack into the reg stack (voxelrcnn_head.py:60-74)
        self.reg_fc_layers, reg_channel = fc_stack(model_cfg['REG_FC'], cls_channel, False)
        self.reg_pred_layer = nn.Linear(reg_channel, self.box_coder.code_size * self.num_class, bias=True)
        self.init_weights()

    def init_weights(self):
        for module_list in [self.shared_fc_layer, self.cls_fc_layers, self.reg_fc_layers]:
            for m in module_list.modules():
                if isinstance(m, nn.Linear):
                    nn.init.xavier_normal_(m.weight)
                    if m.bias is not None:
                        nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.cls_pred_layer.weight, 0, 0.01)
        nn.init.constant_(self.cls_pred_layer.bias, 0)
        nn.init.normal_(self.reg_pred_layer.weight, mean=0, std=0.001)
        nn.init.constant_(self.reg_pred_layer.bias, 0)

    def roi_grid_pool(self, batch_dict):
        """rois (B, num_rois, 7), multi_scale_3d_features / _strides -> (B * num_rois, GRID_SIZE^3, C)."""
        rois = batch_dict['rois']
        batch_size = batch_dict['batch_size']
        with_vf_transform = batch_dict.get('with_voxel_feature_transform', False)
        grid_size = self.pool_cfg['GRID_SIZE']

        roi_grid_xyz, _ = self.get_global_grid_points_of_roi(rois, grid_size=grid_size)        # (BxN, 6x6x6, 3)
        roi_grid_xyz = roi_grid_xyz.view(batch_size, -1, 3)

        roi_grid_coords_x = (roi_grid_xyz[:, :, 0:1] - self.point_cloud_range[0]) // self.voxel_size[0]
        roi_grid_coords_y = (roi_grid_xyz[:, :, 1:2] - self.point_cloud_range[1]) // self.voxel_size[1]
        roi_grid_coords_z = (roi_grid_xyz[:, :, 2:3] - self.point_cloud_range[2]) // self.voxel_size[2]
        roi_grid_coords = torch.cat([roi_grid_coords_x, roi_grid_coords_y, roi_grid_coords_z], dim=-1)

        scenes = torch.arange(batch_size, device=rois.device)
        batch_idx = scenes.to(rois.dtype).view(batch_size, 1, 1).expand(batch_size, roi_grid_coords.shape[1], 1)
        roi_grid_batch_cnt = torch.full((batch_size,), roi_grid_coords.shape[1], dtype=torch.int32, device=rois.device)
        new_xyz = roi_grid_xyz.contiguous().view(-1, 3)

        pooled_features_list = []
        features_key = 'multi_scale_3d_features_post' if with_vf_transform else 'multi_scale_3d_features'
        for k, src_name in enumerate(self.pool_cfg['FEATURES_SOURCE']):
            pool_layer = self.roi_grid_pool_layers[k]
            cur_stride = batch_dict['multi_scale_3d_strides'][src_name]
            cur_sp_tensors = batch_dict[features_key][src_name]

            cur_coords = cur_sp_tensors.indices
            cur_voxel_xyz = get_voxel_centers(cur_coords[:, 1:4], downsample_times=cur_stride, voxel_size=self.voxel_size,
                                              point_cloud_range=self.point_cloud_range)
            cur_voxel_xyz_batch_cnt = (cur_coords[:, 0:1] == scenes[None, :]).sum(dim=0).int()
            v2p_ind_tensor = generate_voxel2pinds(cur_sp_tensors)
            cur_roi_grid_coords = roi_grid_coords // cur_stride
            cur_roi_grid_coords = torch.cat([batch_idx, cur_roi_grid_coords], dim=-1).int()

            pooled_features = pool_layer(
                xyz=cur_voxel_xyz.contiguous(), xyz_batch_cnt=cur_voxel_xyz_batch_cnt, new_xyz=new_xyz,
                new_xyz_batch_cnt=roi_grid_batch_cnt, new_coords=cur_roi_grid_coords.contiguous().view(-1, 4),
                features=cur_sp_tensors.features.contiguous(), voxel2point_indices=v2p_ind_tensor)
            pooled_features_list.append(pooled_features.view(-1, grid_size ** 3, pooled_features.shape[-1]))
        return torch.cat(pooled_features_list, dim=-1)

    def forward(self, batch_dict):
        targets_dict = self.proposals_and_targets(batch_dict)

        pooled_features = self.roi_grid_pool(batch_dict)                                         # (BxN, 6x6x6, C)
        pooled_features = pooled_features.view(pooled_features.size(0), -1)
        shared_features = self.shared_fc_layer(pooled_features)
        rcnn_cls = self.cls_pred_layer(self.cls_fc_layers(shared_features))
        rcnn_reg = self.reg_pred_layer(self.reg_fc_layers(shared_features))

        return self.keep_predictions(batch_dict, targets_dict, rcnn_cls, rcnn_reg)
