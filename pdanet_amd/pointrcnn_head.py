"""PointRCNNHead (pcdet/models/roi_heads/pointrcnn_head.py) for kitti_models/pointrcnn.yaml: the points of each RoI pooled
into its canonical frame, a PointNet++ encoder over them and two fc stacks, under the reference's module names (xyz_up_layer,
merge_down_layer, SA_modules, cls_layers, reg_layers), so a reference checkpoint loads with strict=True.

roipool3d_gpu: the reference builds the head's input from a norm, a cat, enlarge_box3d, two zero fills, the pooling kernel, a
strided subtraction, rotate_points_along_z and a masked zero.  Here `roipoint_pool3d_canonical` (csrc/roi_pool.hip) writes the
(B, M, S, 5 + C) tensor in one launch; its arithmetic is stated in include/pda_train.h.  PDA_ROIPOINT_POOL=composed selects the
reference's composition over RoIPointPool3d instead (the benchmark's baseline, benchmarks/pointrcnn.py).  The points must be
scene-major with equally many rows per scene (the reference asserts the same); the count comes from the shape.  Nothing of the
pooled tensor requires grad, as in the reference.

The SA stack runs through PointnetSAModule, whose `bn` argument the reference ignores: its layers keep their BatchNorm with
USE_BN: False, only xyz_up_layer and merge_down_layer follow the key.  The losses are the template's.

Target sampling: batch_dict may carry 'roi_target_seed' or 'roi_target_draws' (ProposalTargetLayer.forward's seed / draws).

Out of scope: boxes with velocities, a backward for the pooling, graph capture of the head."""
from functools import partial

import torch
import torch.nn as nn

from . import pointnet2_modules, roipoint_pool3d_utils
from .config import fused_or_composed
from .roi_head_template import RoIHeadTemplate

# 'fused' (default) or 'composed', read when the head pools
ENV = "PDA_ROIPOINT_POOL"
pool_path = partial(fused_or_composed, ENV)


class PointRCNNHead(RoIHeadTemplate):
    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        use_bn = model_cfg['USE_BN']
        self.SA_modules = nn.ModuleList()
        channel_in = input_channels

        self.num_prefix_channels = 3 + 2                                   # xyz + point_scores + point_depth
        xyz_mlps = [self.num_prefix_channels] + list(model_cfg['XYZ_UP_LAYER'])
        shared_mlps = []
        for k in range(len(xyz_mlps) - 1):
            shared_mlps.append(nn.Conv2d(xyz_mlps[k], xyz_mlps[k + 1], kernel_size=1, bias=not use_bn))
            if use_bn:
                shared_mlps.append(nn.BatchNorm2d(xyz_mlps[k + 1]))
            shared_mlps.append(nn.ReLU())
        self.xyz_up_layer = nn.Sequential(*shared_mlps)

        c_out = model_cfg['XYZ_UP_LAYER'][-1]
        self.merge_down_layer = nn.Sequential(nn.Conv2d(c_out * 2, c_out, kernel_size=1, bias=not use_bn),
                                              *([nn.BatchNorm2d(c_out), nn.ReLU()] if use_bn else [nn.ReLU()]))

        sa_cfg = model_cfg['SA_CONFIG']
        for k in range(len(sa_cfg['NPOINTS'])):
            mlps = [channel_in] + list(sa_cfg['MLPS'][k])
            npoint = sa_cfg['NPOINTS'][k] if sa_cfg['NPOINTS'][k] != -1 else None
            self.SA_modules.append(pointnet2_modules.PointnetSAModule(npoint=npoint, radius=sa_cfg['RADIUS'][k],
                                                                      nsample=sa_cfg['NSAMPLE'][k], mlp=mlps, use_xyz=True, bn=use_bn))
            channel_in = mlps[-1]

        self.cls_layers = self.make_fc_layers(input_channels=channel_in, output_channels=self.num_class, fc_list=model_cfg['CLS_FC'])
        self.reg_layers = self.make_fc_layers(input_channels=channel_in, output_channels=self.box_coder.code_size * self.num_class,
                                              fc_list=model_cfg['REG_FC'])
        pool_cfg = model_cfg['ROI_POINT_POOL']
        self.roipoint_pool3d_layer = roipoint_pool3d_utils.RoIPointPool3d(num_sampled_points=pool_cfg['NUM_SAMPLED_POINTS'],
                                                                          pool_extra_width=pool_cfg['POOL_EXTRA_WIDTH'])
        self.init_weights(weight_init='xavier')

    def roipool3d_gpu(self, batch_dict):
        """rois (B, num_rois, 7), point_coords (B * N, 4) [bs_idx, x, y, z], point_features (B * N, C), point_cls_scores (B * N)
        -> (B * num_rois, NUM_SAMPLED_POINTS, 5 + C): [canonical xyz | score | depth | features], zero for an empty RoI."""
        batch_size = batch_dict['batch_size']
        rois = batch_dict['rois']
        if rois.shape[-1] > 7:
            raise NotImplementedError("boxes with velocities are not supported")
        point_coords = batch_dict['point_coords'][:, 1:4]
        if point_coords.shape[0] % batch_size != 0:
            raise ValueError("roipool3d_gpu needs equally many points per scene, got %d rows for %d scenes"
                             % (point_coords.shape[0], batch_size))
        batch_points = point_coords.reshape(batch_size, -1, 3)
        point_features = batch_dict['point_features']
        point_features = point_features.reshape(batch_size, -1, point_features.shape[-1])
        point_scores = batch_dict['point_cls_scores'].reshape(batch_size, -1)
        pool_cfg = self.model_cfg['ROI_POINT_POOL']
        pool = (roipoint_pool3d_utils.roipoint_pool3d_canonical if pool_path() == "fused"
                else roipoint_pool3d_utils.roipoint_pool3d_canonical_composed)
        pooled_features, _ = pool(batch_points, point_scores, point_features, rois, pool_cfg['POOL_EXTRA_WIDTH'],
                                  pool_cfg['NUM_SAMPLED_POINTS'], pool_cfg['DEPTH_NORMALIZER'])
        return pooled_features.view(-1, pooled_features.shape[-2], pooled_features.shape[-1])

    def forward(self, batch_dict):
        targets_dict = self.proposals_and_targets(batch_dict)

        pooled_features = self.roipool3d_gpu(batch_dict)                    # (total_rois, num_sampled_points, 5 + C)

        xyz_input = pooled_features[..., 0:self.num_prefix_channels].transpose(1, 2).unsqueeze(dim=3).contiguous()
        xyz_features = self.xyz_up_layer(xyz_input)
        point_features = pooled_features[..., self.num_prefix_channels:].transpose(1, 2).unsqueeze(dim=3)
        merged_features = self.merge_down_layer(torch.cat((xyz_features, point_features), dim=1))

        l_xyz, l_features = [pooled_features[..., 0:3].contiguous()], [merged_features.squeeze(dim=3).contiguous()]
        for i in range(len(self.SA_modules)):
            li_xyz, li_features = self.SA_modules[i](l_xyz[i], l_features[i])
            l_xyz.append(li_xyz)
            l_features.append(li_features)

        shared_features = l_features[-1]                                    # (total_rois, num_features, 1)
        rcnn_cls = self.cls_layers(shared_features).transpose(1, 2).contiguous().squeeze(dim=1)   # (B, 1 or 2)
        rcnn_reg = self.reg_layers(shared_features).transpose(1, 2).contiguous().squeeze(dim=1)   # (B, C)

        return self.keep_predictions(batch_dict, targets_dict, rcnn_cls, rcnn_reg)
