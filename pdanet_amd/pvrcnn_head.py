"""PVRCNNHead (pcdet/models/roi_heads/pvrcnn_head.py): RoI-grid pooling of the keypoint features
(pointnet2_stack_modules.StackSAModuleMSG, fused in csrc/stack_sa.hip), the Conv1d shared stack and the two prediction stacks
of RoIHeadTemplate.make_fc_layers, the rcnn losses of RoIHeadTemplate -- under the reference's module names
(roi_grid_pool_layer, shared_fc_layer, cls_layers, reg_layers), so a reference checkpoint loads with strict=True.

The grid-point arithmetic is the reference's torch expressions.  Where the reference counts the keypoints per scene in a
Python loop and builds the grid index with nonzero(), this compares against an arange and builds the index grid directly:
the training path reads nothing on the host.  The model config is not modified (the reference prepends the input channels to
ROI_GRID_POOL.MLPS in place).

The RoIs are detached targets or first-stage proposals: the grid points carry no gradient (pointnet2_stack_modules).

Target sampling: batch_dict may carry 'roi_target_seed' or 'roi_target_draws' (ProposalTargetLayer.forward's seed / draws).

Out of scope: graph capture of the head."""
import torch
import torch.nn as nn

from . import box_utils
from .pointnet2_stack_modules import build_local_aggregation_module
from .roi_head_template import RoIHeadTemplate
from .voxel_set_abstraction import scene_counts


class PVRCNNHead(RoIHeadTemplate):
    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.pool_cfg = model_cfg['ROI_GRID_POOL']
        self.roi_grid_pool_layer, num_c_out = build_local_aggregation_module(input_channels=input_channels, config=self.pool_cfg)

        grid = self.pool_cfg['GRID_SIZE']
        pre_channel = grid * grid * grid * num_c_out
        shared_fc_list = []
        widths = model_cfg['SHARED_FC']
        for k in range(len(widths)):
            shared_fc_list.extend([nn.Conv1d(pre_channel, widths[k], kernel_size=1, bias=False), nn.BatchNorm1d(widths[k]),
                                   nn.ReLU()])
            pre_channel = widths[k]
            if k != len(widths) - 1 and model_cfg['DP_RATIO'] > 0:
                shared_fc_list.append(nn.Dropout(model_cfg['DP_RATIO']))
        self.shared_fc_layer = nn.Sequential(*shared_fc_list)
        self.cls_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=self.num_class,
                                              fc_list=model_cfg['CLS_FC'])
        self.reg_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=self.box_coder.code_size * self.num_class,
                                              fc_list=model_cfg['REG_FC'])
        self.init_weights(weight_init='xavier')

    def init_weights(self, weight_init='xavier'):
        if weight_init == 'kaiming':
            init_func = nn.init.kaiming_normal_
        elif weight_init == 'xavier':
            init_func = nn.init.xavier_normal_
        elif weight_init == 'normal':
            init_func = nn.init.normal_
        else:
            raise NotImplementedError
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                if weight_init == 'normal':
                    init_func(m.weight, mean=0, std=0.001)
                else:
                    init_func(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)

    def roi_grid_pool(self, batch_dict):
        """rois (B, num_rois, 7 + C), point_coords (P, 4) [bs_idx, x, y, z], point_features (P, C), point_cls_scores (P)
        -> (B * num_rois, GRID_SIZE^3, C_out)."""
        batch_size = batch_dict['batch_size']
        rois = batch_dict['rois']
        point_coords = batch_dict['point_coords']
        point_features = batch_dict['point_features'] * batch_dict['point_cls_scores'].view(-1, 1)
        grid_size = self.pool_cfg['GRID_SIZE']

        global_roi_grid_points, _ = self.get_global_grid_points_of_roi(rois, grid_size=grid_size)      # (BxN, 6x6x6, 3)
        global_roi_grid_points = global_roi_grid_points.view(batch_size, -1, 3)                          # (B, Nx6x6x6, 3)

        xyz = point_coords[:, 1:4]
        xyz_batch_cnt = scene_counts(point_coords[:, 0], batch_size)
        new_xyz = global_roi_grid_points.view(-1, 3)
        new_xyz_batch_cnt = torch.full((batch_size,), global_roi_grid_points.shape[1], dtype=torch.int32, device=xyz.device)
        _, pooled_features = self.roi_grid_pool_layer(xyz=xyz.contiguous(), xyz_batch_cnt=xyz_batch_cnt, new_xyz=new_xyz.contiguous(),
                                                      new_xyz_batch_cnt=new_xyz_batch_cnt, features=point_features.contiguous())
        return pooled_features.view(-1, grid_size ** 3, pooled_features.shape[-1])                        # (BxN, 6x6x6, C)

    def get_global_grid_points_of_roi(self, rois, grid_size):
        rois = rois.view(-1, rois.shape[-1])
        batch_size_rcnn = rois.shape[0]
        local_roi_grid_points = self.get_dense_grid_points(rois, batch_size_rcnn, grid_size)            # (B, 6x6x6, 3)
        global_roi_grid_points = box_utils.rotate_points_along_z(local_roi_grid_points.clone(), rois[:, 6]).squeeze(dim=1)
        global_center = rois[:, 0:3].clone()
        global_roi_grid_points += global_center.unsqueeze(dim=1)
        return global_roi_grid_points, local_roi_grid_points

    @staticmethod
    def get_dense_grid_points(rois, batch_size_rcnn, grid_size):
        """The reference's `faked_features.nonzero()` of an all-ones cube is the index grid in row-major order; built here
        without the host read nonzero() makes."""
        axis = torch.arange(grid_size, device=rois.device)
        dense_idx = torch.stack(torch.meshgrid(axis, axis, axis, indexing='ij'), dim=-1).view(-1, 3)
        dense_idx = dense_idx.repeat(batch_size_rcnn, 1, 1).to(rois.dtype)                               # (B, 6x6x6, 3)
        local_roi_size = rois.view(batch_size_rcnn, -1)[:, 3:6]
        roi_grid_points = (dense_idx + 0.5) / grid_size * local_roi_size.unsqueeze(dim=1) \
            - (local_roi_size.unsqueeze(dim=1) / 2)
        return roi_grid_points

    def forward(self, batch_dict):
        targets_dict = self.proposal_layer(batch_dict, nms_config=self.model_cfg['NMS_CONFIG']['TRAIN' if self.training else 'TEST'])
        if self.training:
            targets_dict = batch_dict.get('roi_targets_dict', None)
            if targets_dict is None:
                targets_dict = self.assign_targets(batch_dict, seed=batch_dict.get('roi_target_seed'),
                                                   draws=batch_dict.get('roi_target_draws'))
                batch_dict['rois'] = targets_dict['rois']
                batch_dict['roi_labels'] = targets_dict['roi_labels']

        pooled_features = self.roi_grid_pool(batch_dict)                                                 # (BxN, 6x6x6, C)
        batch_size_rcnn = pooled_features.shape[0]
        pooled_features = pooled_features.permute(0, 2, 1).contiguous()                                  # (BxN, C, 6x6x6)
        shared_features = self.shared_fc_layer(pooled_features.view(batch_size_rcnn, -1, 1))
        rcnn_cls = self.cls_layers(shared_features).transpose(1, 2).contiguous().squeeze(dim=1)          # (B, 1 or 2)
        rcnn_reg = self.reg_layers(shared_features).transpose(1, 2).contiguous().squeeze(dim=1)          # (B, C)

        if not self.training:
            batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(
                batch_size=batch_dict['batch_size'], rois=batch_dict['rois'], cls_preds=rcnn_cls, box_preds=rcnn_reg)
            batch_dict['batch_cls_preds'] = batch_cls_preds
            batch_dict['batch_box_preds'] = batch_box_preds
            batch_dict['cls_preds_normalized'] = False
        else:
            targets_dict['rcnn_cls'] = rcnn_cls
            targets_dict['rcnn_reg'] = rcnn_reg
            self.forward_ret_dict = targets_dict
        return batch_dict
