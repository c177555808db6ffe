"""The reference's dynamic voxel feature encoders on the device: DynamicMeanVFE, DynamicPillarVFE and PFNLayerV2
(pcdet/models/backbones_3d/vfe/dynamic_mean_vfe.py, dynamic_pillar_vfe.py), with their constructor signatures, config keys,
state-dict keys (pfn_layers.{i}.linear.weight, pfn_layers.{i}.norm.*) and batch_dict contract, so a reference checkpoint
loads unchanged.  torch.unique and torch_scatter are replaced by the operators of dyn_voxel_utils.py; Linear, BatchNorm1d
and the x_max[unq_inv] gather stay in torch.

The reference's output shapes depend on the data, so each forward does exactly ONE host read: the two counts
[n_kept, n_voxels], right after the index stage; the padded tensors are then sliced.  The operators underneath read nothing
back.

One departure from the reference: the float32 sums of scatter_mean run in ascending point order (torch_scatter's atomic
order is not defined), and batch_size * cells >= 2^31 is refused where the reference's int32 merge_coords wraps.
"""
import torch
import torch.nn as nn

from . import dyn_voxel_utils as dvu
from .config import field


class _Sliced:
    """A DynVoxelIndex cut to its live counts (host integers) for the layers of one forward."""

    def __init__(self, index):
        self.index = index
        self.n_kept, self.n_voxels = (int(v) for v in index.counts.tolist())      # the forward's one host read
        self.point_idx = index.point_idx[:self.n_kept].long()
        self.unq_inv = index.unq_inv[:self.n_kept].long()
        self.voxel_coords = index.voxel_coords[:self.n_voxels]


class VFETemplate(nn.Module):
    def __init__(self, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg

    def get_output_feature_dim(self):
        raise NotImplementedError

    def forward(self, **kwargs):
        raise NotImplementedError


class PFNLayerV2(nn.Module):
    def __init__(self, in_channels, out_channels, use_norm=True, last_layer=False):
        super().__init__()
        self.last_vfe = last_layer
        self.use_norm = use_norm
        if not self.last_vfe:
            out_channels = out_channels // 2
        if self.use_norm:
            self.linear = nn.Linear(in_channels, out_channels, bias=False)
            self.norm = nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01)
        else:
            self.linear = nn.Linear(in_channels, out_channels, bias=True)
        self.relu = nn.ReLU()

    def forward(self, inputs, sliced):
        """inputs (n_kept, in_channels); sliced: the _Sliced index of this forward (the reference passes unq_inv)."""
        x = self.linear(inputs)
        x = self.norm(x) if self.use_norm else x
        x = self.relu(x)
        x_max, _ = dvu.ScatterMax.apply(x.contiguous(), sliced.index, sliced.n_voxels)
        if self.last_vfe:
            return x_max
        return torch.cat([x, x_max[sliced.unq_inv, :]], dim=1)


class DynamicPillarVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, grid_size, point_cloud_range, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.use_norm = field(model_cfg, "USE_NORM")
        self.with_distance = field(model_cfg, "WITH_DISTANCE")
        self.use_absolute_xyz = field(model_cfg, "USE_ABSLOTE_XYZ")
        num_point_features += 6 if self.use_absolute_xyz else 3
        if self.with_distance:
            num_point_features += 1
        self.num_filters = field(model_cfg, "NUM_FILTERS")
        assert len(self.num_filters) > 0
        num_filters = [num_point_features] + list(self.num_filters)
        self.pfn_layers = nn.ModuleList(
            PFNLayerV2(num_filters[i], num_filters[i + 1], self.use_norm, last_layer=(i >= len(num_filters) - 2))
            for i in range(len(num_filters) - 1))
        self.spec = dvu.DynVoxelSpec(point_cloud_range, voxel_size, grid_size)

    def get_output_feature_dim(self):
        return self.num_filters[-1]

    def forward(self, batch_dict, **kwargs):
        """batch_dict['points'] (n, 1 + C) [batch_idx, x, y, z, ...], batch_dict['batch_size'] -> 'pillar_features'
        (n_pillars, NUM_FILTERS[-1]) and 'voxel_coords' (n_pillars, 4) int32 (b, 0, y, x), pillars in ascending order of
        merge_coords.  One host read (the two counts)."""
        points = batch_dict["points"].contiguous()
        index = dvu.dynamic_voxel_index(points.detach(), self.spec, batch_dict["batch_size"], pillars=True)
        mean = dvu.scatter_mean(points.detach()[:, 1:4][index.point_idx.long()], index)
        features = dvu.PillarFeatures.apply(points, index, mean, self.spec, self.use_absolute_xyz, self.with_distance)
        sliced = _Sliced(index)
        features = features[:sliced.n_kept]
        for pfn in self.pfn_layers:
            features = pfn(features, sliced)
        batch_dict["pillar_features"] = features
        batch_dict["voxel_coords"] = sliced.voxel_coords
        return batch_dict


class DynamicMeanVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, grid_size, point_cloud_range, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.num_point_features = num_point_features
        self.spec = dvu.DynVoxelSpec(point_cloud_range, voxel_size, grid_size)

    def get_output_feature_dim(self):
        return self.num_point_features

    @torch.no_grad()
    def forward(self, batch_dict, **kwargs):
        """batch_dict['points'] (n, 1 + C), batch_dict['batch_size'] -> 'voxel_features' (n_voxels, C), the mean of the
        voxel's points[:, 1:], and 'voxel_coords' (n_voxels, 4) int32 (b, z, y, x), voxels in ascending order of
        merge_coords.  One host read (the two counts)."""
        points = batch_dict["points"].contiguous()
        index = dvu.dynamic_voxel_index(points, self.spec, batch_dict["batch_size"], pillars=False)
        sliced = _Sliced(index)
        data = points[:, 1:][sliced.point_idx].contiguous()
        batch_dict["voxel_features"] = dvu.scatter_mean(data, index, sliced.n_voxels)
        batch_dict["voxel_coords"] = sliced.voxel_coords.contiguous()
        return batch_dict
