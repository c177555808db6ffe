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

from .pointnet2_stack_modules import build_local_aggregation_module
from .roi_head_template import RoIHeadTemplate
from .voxel_set_abstraction import scene_counts


class PVRCNNHead(RoIHeadTemplate):
    build_local_aggregation_module = staticmethod(build_local_aggregation_module)     # pv_rcnn_plusplus.py names another

    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.pool_cfg = model_cfg['ROI_GRID_POOL']
        self.roi_grid_pool_layer, num_c_out = self.build_local_aggregation_module(input_channels=input_channels, config=self.pool_cfg)

        grid = self.pool_cfg['GRID_SIZE']
        self.shared_fc_layer, pre_channel = self.make_shared_fc_layers(grid * grid * grid * num_c_out, model_cfg['SHARED_FC'])
        self.cls_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=self.num_class,
                                              fc_list=model_cfg['CLS_FC'])
        self.reg_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=self.box_coder.code_size * self.num_class,
                                              fc_list=model_cfg['REG_FC'])
        self.init_weights(weight_init='xavier')

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

    def forward(self, batch_dict):
        # sampled targets a caller made already (with their rois in the batch) are taken as they are
        targets_dict = batch_dict.get('roi_targets_dict', None) if self.training else None
        if targets_dict is None:
            targets_dict = self.proposals_and_targets(batch_dict)

        pooled_features = self.roi_grid_pool(batch_dict)                                                 # (BxN, 6x6x6, C)
        batch_size_rcnn = pooled_features.shape[0]
        pooled_features = pooled_features.permute(0, 2, 1).contiguous()                                  # (BxN, C, 6x6x6)
        shared_features = self.shared_fc_layer(pooled_features.view(batch_size_rcnn, -1, 1))
        rcnn_cls = self.cls_layers(shared_features).transpose(1, 2).contiguous().squeeze(dim=1)          # (B, 1 or 2)
        rcnn_reg = self.reg_layers(shared_features).transpose(1, 2).contiguous().squeeze(dim=1)          # (B, C)

        return self.keep_predictions(batch_dict, targets_dict, rcnn_cls, rcnn_reg)
