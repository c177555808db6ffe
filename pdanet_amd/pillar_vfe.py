"""The hard-voxel PillarVFE and PFNLayer of PointPillar (pcdet/models/backbones_3d/vfe/pillar_vfe.py) with the reference's
constructor signatures, config keys (USE_NORM, WITH_DISTANCE, USE_ABSLOTE_XYZ, NUM_FILTERS), state-dict keys
(pfn_layers.{i}.linear.weight, pfn_layers.{i}.norm.*) and batch_dict contract.  The PFN input rows -- raw columns,
offsets from the voxel's mean and from the cell centre, the padding mask -- are one launch of csrc/pillar.hip
(pda_pillar_features) where the reference makes about a dozen passes; Linear, BatchNorm1d, ReLU and the max over the points
stay in torch.  Voxels are data: there is no backward into them.

One departure from the reference: the float32 sum behind the mean runs in row order (torch's own order over the P rows is
not defined), so the xyz - mean columns agree within the bound of two summation orders, not bit for bit."""
import ctypes

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .config import field
from .dynamic_vfe import VFETemplate
from .pointnet2_batch_cuda import F32, I32, _call, _chk


def pillar_features(voxels, voxel_num_points, voxel_coords, voxel_size, point_cloud_range, use_absolute_xyz=True,
                    with_distance=False):
    """voxels (V, P, C) float32, voxel_num_points (V) int, voxel_coords (V, 4) int (b, z, y, x) -> (V, P, C') with
    C' = (C or C - 3) + 6 (+ 1): [raw columns, xyz - mean, xyz - cell centre, (|xyz|)], rows from num_points on exactly 0."""
    if isinstance(voxels, torch.Tensor) and voxels.requires_grad:
        raise RuntimeError("voxels are data: pillar_features has no backward")
    if not isinstance(voxels, torch.Tensor) or voxels.dim() != 3 or voxels.shape[2] < 3:
        raise ValueError("voxels must be a (V, P, C >= 3) tensor")
    _chk(voxels, "voxels", F32)
    V, P, C = voxels.shape
    num = voxel_num_points if voxel_num_points.dtype == I32 else voxel_num_points.to(I32)
    crd = voxel_coords if voxel_coords.dtype == I32 else voxel_coords.to(I32)
    num, crd = num.contiguous(), crd.contiguous()
    _chk(num, "voxel_num_points", I32), _chk(crd, "voxel_coords", I32)
    if num.numel() != V or tuple(crd.shape) != (V, 4):
        raise ValueError("voxel_num_points must be (V) and voxel_coords (V, 4)")
    vs = [float(v) for v in voxel_size]
    lo = [float(v) for v in point_cloud_range[:3]]
    vs_c = (ctypes.c_float * 3)(*vs)
    off_c = (ctypes.c_float * 3)(*[vs[i] / 2 + lo[i] for i in range(3)])       # float64 sums, rounded once, as the reference
    c_out = (C if use_absolute_xyz else C - 3) + 6 + (1 if with_distance else 0)
    out = torch.empty((V, P, c_out), dtype=F32, device=voxels.device)
    if V * P:
        _call("pda_pillar_features", voxels, voxels.data_ptr(), num.data_ptr(), crd.data_ptr(), V, P, C, vs_c, off_c,
              int(bool(use_absolute_xyz)), int(bool(with_distance)), out.data_ptr())
    return out


class PFNLayer(nn.Module):
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

    def forward(self, inputs):
        """inputs (V, P, in_channels) -> (V, 1, out) for the last layer, (V, P, 2 * out) otherwise."""
        x = self.linear(inputs)
        if self.use_norm:
            x = self.norm(x.permute(0, 2, 1)).permute(0, 2, 1)
        x = F.relu(x)
        x_max = torch.max(x, dim=1, keepdim=True)[0]
        if self.last_vfe:
            return x_max
        return torch.cat([x, x_max.expand(-1, inputs.shape[1], -1)], dim=2)


class PillarVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, point_cloud_range, **kwargs):
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
            PFNLayer(num_filters[i], num_filters[i + 1], self.use_norm, last_layer=(i >= len(num_filters) - 2))
            for i in range(len(num_filters) - 1))
        self.voxel_size = [float(v) for v in np.asarray(voxel_size).tolist()]
        self.point_cloud_range = [float(v) for v in np.asarray(point_cloud_range).tolist()]

    def get_output_feature_dim(self):
        return self.num_filters[-1]

    def forward(self, batch_dict, **kwargs):
        """batch_dict['voxels'] (V, P, C), 'voxel_num_points' (V), 'voxel_coords' (V, 4) (b, z, y, x) -> 'pillar_features'
        (V, NUM_FILTERS[-1]).  No host read."""
        features = pillar_features(batch_dict['voxels'], batch_dict['voxel_num_points'], batch_dict['voxel_coords'],
                                   self.voxel_size, self.point_cloud_range, self.use_absolute_xyz, self.with_distance)
        for pfn in self.pfn_layers:
            features = pfn(features)
        batch_dict['pillar_features'] = features.squeeze(1)      # the reference's squeeze() also drops V == 1
        return batch_dict
