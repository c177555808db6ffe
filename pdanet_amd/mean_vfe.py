"""MeanVFE (pcdet/models/backbones_3d/vfe/mean_vfe.py): the mean of a hard voxel's points, a few torch operations."""
import torch
import torch.nn as nn


class MeanVFE(nn.Module):
    def __init__(self, model_cfg, num_point_features, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_point_features = num_point_features

    def get_output_feature_dim(self):
        return self.num_point_features

    def forward(self, batch_dict, **kwargs):
        """voxels (num_voxels, max_points_per_voxel, C), voxel_num_points (num_voxels) -> voxel_features (num_voxels, C).
        A padded batch (voxel_num_active, voxel_status: voxel_utils.collate_voxels_padded) passes through as it is: a dead
        row has zero points and zero voxels, so its mean is 0 / 1 = 0."""
        voxel_features, voxel_num_points = batch_dict['voxels'], batch_dict['voxel_num_points']
        points_mean = voxel_features.sum(dim=1, keepdim=False)
        normalizer = torch.clamp_min(voxel_num_points.view(-1, 1), min=1.0).type_as(voxel_features)
        batch_dict['voxel_features'] = (points_mean / normalizer).contiguous()
        return batch_dict
