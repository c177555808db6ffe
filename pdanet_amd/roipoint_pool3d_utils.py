"""Mirror of pcdet/ops/roipoint_pool3d (roipoint_pool3d_utils.py:9-63 over roipoint_pool3d_cuda.forward,
src/roipoint_pool3d.cpp:23-58) on libpda_pointnet2.so (include/pda_train.h, csrc/roi_pool.hip): the point pooling of the
PointRCNN head, and that head's whole input stage as one launch (roipoint_pool3d_canonical) next to the reference's
composition of it (roipoint_pool3d_canonical_composed)."""
import ctypes

import torch
import torch.nn as nn
from torch.autograd import Function

from . import box_utils
from .pointnet2_batch_cuda import F32, I32, _call, _chk, _numel_ok


class roipoint_pool3d_cuda:  # noqa: N801  (the reference's extension module name)
    @staticmethod
    def forward(xyz, boxes3d, pts_feature, pooled_features, pooled_empty_flag):
        """xyz (B,P,3), boxes3d (B,M,7) already enlarged, pts_feature (B,P,C) -> pooled_features (B,M,S,3+C),
        pooled_empty_flag (B,M) int32, both zero-filled by the caller; sizes come from the tensors -> 1."""
        b, p, m, c, s = xyz.shape[0], xyz.shape[1], boxes3d.shape[1], pts_feature.shape[2], pooled_features.shape[2]
        _numel_ok(xyz, b * p * 3, "xyz"); _numel_ok(boxes3d, b * m * 7, "boxes3d"); _numel_ok(pts_feature, b * p * c, "pts_feature")
        _numel_ok(pooled_features, b * m * s * (3 + c), "pooled_features"); _numel_ok(pooled_empty_flag, b * m, "pooled_empty_flag")
        _call("pda_roipoint_pool3d_fwd", xyz, _chk(xyz, "xyz", F32), _chk(boxes3d, "boxes3d", F32), _chk(pts_feature, "pts_feature", F32),
              _chk(pooled_features, "pooled_features", F32), _chk(pooled_empty_flag, "pooled_empty_flag", I32), b, p, m, c, s)
        if p == 0:
            pooled_empty_flag.fill_(1)             # the library leaves an empty problem alone; every box is empty
        return 1


def _extra_width(pool_extra_width):
    return (pool_extra_width,) * 3 if isinstance(pool_extra_width, (int, float)) else tuple(pool_extra_width)


def roipoint_pool3d_canonical(points, point_scores, point_features, rois, pool_extra_width, num_sampled_points, depth_normalizer):
    """MI355X extension (csrc/roi_pool.hip, pda_roipoint_pool3d_canonical_fwd): PointRCNNHead.roipool3d_gpu in one launch.
    points (B, N, 3), point_scores (B, N), point_features (B, N, C), rois (B, M, 7) not enlarged ->
    pooled (B, M, S, 5 + C) rows [canonical xyz | score | depth | features], the blocks of empty RoIs zero, and
    pooled_empty_flag (B, M) int32.  Neither requires grad: the reference pools under no_grad."""
    if points.dim() != 3 or points.shape[2] != 3 or rois.dim() != 3 or rois.shape[2] != 7 or rois.shape[0] != points.shape[0]:
        raise ValueError("points must be (B, N, 3) and rois (B, M, 7), got %s and %s" % (tuple(points.shape), tuple(rois.shape)))
    points, rois = points.detach().contiguous(), rois.detach().contiguous()
    point_scores, point_features = point_scores.detach().contiguous(), point_features.detach().contiguous()
    b, n, m, c, s = points.shape[0], points.shape[1], rois.shape[1], point_features.shape[-1], int(num_sampled_points)
    _numel_ok(point_scores, b * n, "point_scores"); _numel_ok(point_features, b * n * c, "point_features")
    extra = (ctypes.c_float * 3)(*[float(w) for w in _extra_width(pool_extra_width)])
    ptrs = [_chk(t, name, F32) for t, name in ((points, "points"), (point_scores, "point_scores"),
                                                (point_features, "point_features"), (rois, "rois"))]
    pooled = torch.empty((b, m, s, 5 + c), dtype=F32, device=points.device)
    flag = torch.empty((b, m), dtype=I32, device=points.device)
    _call("pda_roipoint_pool3d_canonical_fwd", points, *ptrs, extra, float(depth_normalizer), _chk(pooled, "pooled", F32),
          _chk(flag, "pooled_empty_flag", I32), b, n, m, c, s)
    return pooled, flag


def roipoint_pool3d_canonical_composed(points, point_scores, point_features, rois, pool_extra_width, num_sampled_points,
                                       depth_normalizer):
    """The reference's composition of the same tensors (pointrcnn_head.py:109-129) over RoIPointPool3d: norm, cat, enlarge,
    two zero fills, the pooling kernel, the subtraction of the centre, rotate_points_along_z and the masked zero."""
    with torch.no_grad():
        points, rois = points.detach(), rois.detach()
        depths = points.norm(dim=2) / depth_normalizer - 0.5
        features_all = torch.cat([point_scores.detach().unsqueeze(-1), depths.unsqueeze(-1), point_features.detach()], dim=2)
        pooled, flag = RoIPointPool3dFunction.apply(points, features_all, rois, pool_extra_width, int(num_sampled_points))
        pooled[:, :, :, 0:3] -= rois[:, :, 0:3].unsqueeze(dim=2)
        flat = pooled.view(-1, pooled.shape[-2], pooled.shape[-1])
        flat[:, :, 0:3] = box_utils.rotate_points_along_z(flat[:, :, 0:3], -rois.reshape(-1, rois.shape[-1])[:, 6])
        flat.masked_fill_(flag.view(-1, 1, 1) > 0, 0.0)                     # pooled_features[flag > 0] = 0 without the host
    return pooled, flag


class RoIPointPool3d(nn.Module):
    def __init__(self, num_sampled_points=512, pool_extra_width=1.0):
        super().__init__()
        self.num_sampled_points = num_sampled_points
        self.pool_extra_width = pool_extra_width

    def forward(self, points, point_features, boxes3d):
        """
        Args:
            points: (B, N, 3)
            point_features: (B, N, C)
            boxes3d: (B, M, 7), [x, y, z, dx, dy, dz, heading]
        Returns:
            pooled_features: (B, M, num_sampled_points, 3 + C)
            pooled_empty_flag: (B, M)
        """
        return RoIPointPool3dFunction.apply(points, point_features, boxes3d, self.pool_extra_width, self.num_sampled_points)


class RoIPointPool3dFunction(Function):
    @staticmethod
    def forward(ctx, points, point_features, boxes3d, pool_extra_width, num_sampled_points=512):
        """pool_extra_width: one width for the three extents, or (extra_x, extra_y, extra_z)."""
        assert points.shape.__len__() == 3 and points.shape[2] == 3
        batch_size, boxes_num, feature_len = points.shape[0], boxes3d.shape[1], point_features.shape[2]
        width = _extra_width(pool_extra_width)
        pooled_boxes3d = box_utils.enlarge_box3d(boxes3d.view(-1, 7), width).view(batch_size, -1, 7)
        pooled_features = point_features.new_zeros((batch_size, boxes_num, num_sampled_points, 3 + feature_len))
        pooled_empty_flag = point_features.new_zeros((batch_size, boxes_num)).int()
        roipoint_pool3d_cuda.forward(points.contiguous(), pooled_boxes3d.contiguous(), point_features.contiguous(), pooled_features,
                                     pooled_empty_flag)
        return pooled_features, pooled_empty_flag

    @staticmethod
    def backward(ctx, grad_out, grad_flag=None):
        # (autograd hands over one gradient per output; the reference's one-argument form fails with a TypeError before it
        # reaches its own raise)
        raise NotImplementedError
