"""Dynamic voxelization on the device (csrc/dyn_voxel.hip, include/pda_train.h pda_dyn_*): what the reference's dynamic
encoders (pcdet/models/backbones_3d/vfe/dynamic_mean_vfe.py, dynamic_pillar_vfe.py) get from torch.unique and
torch_scatter -- every point inside the grid joins the voxel of its cell, no cap on voxels or on points per voxel.

The operators here do no host read: their outputs are padded to the number of input rows and the live counts stay on the
device (DynVoxelIndex.counts).  dynamic_vfe.py reads the two counts once and slices.
"""
import ctypes

import numpy as np
import torch

from .pointnet2_batch_cuda import F32, I32, _call, _chk
from .stage_common import workspace
from .voxel_utils import grid_size as _grid_size


class DynVoxelSpec:
    """Range, voxel size and grid of a dynamic encoder as C arrays; grid_size as the reference's constructors take it
    (None: rounded from the range, as the dataset computes it).  offset = voxel_size / 2 + range[:3], computed in double
    and rounded to float32 -- what Python does when a float32 tensor expression takes the scalar."""

    def __init__(self, point_cloud_range, voxel_size, grid_size=None):
        pr = np.asarray(point_cloud_range, dtype=np.float64).reshape(-1)
        vs = np.asarray(voxel_size, dtype=np.float64).reshape(-1)
        if pr.shape != (6,) or vs.shape != (3,):
            raise ValueError("point_cloud_range must hold 6 values and the voxel size 3")
        self.grid = np.asarray(_grid_size(pr, vs) if grid_size is None else grid_size, dtype=np.int64).reshape(-1)
        if self.grid.shape != (3,) or (self.grid < 1).any() or (self.grid > 2 ** 24).any():
            raise ValueError("the voxel grid %s is empty or holds more than 2^24 cells along an axis" % (self.grid.tolist(),))
        self.point_cloud_range, self.voxel_size = pr, vs
        offset = vs / 2 + pr[:3]
        self.range_c = (ctypes.c_float * 6)(*pr.tolist())
        self.vsize_c = (ctypes.c_float * 3)(*vs.tolist())
        self.grid_c = (ctypes.c_int32 * 3)(*self.grid.tolist())
        self.offset_c = (ctypes.c_float * 3)(*offset.tolist())

    def key_range(self, batch_size, pillars):
        """batch_size * cells: merge_coords lies in [0, key_range)."""
        g = [int(v) for v in self.grid]
        return int(batch_size) * g[0] * g[1] * (1 if pillars else g[2])


class DynVoxelIndex:
    """The padded outputs of pda_dyn_voxel_index for n input rows (all int32, zero beyond the live counts):
    counts (2) = [n_kept, n_voxels]; point_idx (n) the kept rows, ascending (points[mask]); unq_inv (n) the voxel of a kept
    point = the rank of its key among the sorted distinct keys; unq_cnt (n); voxel_coords (n, 4) = (b, z, y, x), pillars
    (b, 0, y, x); seg_start (n + 1), seg_points (n): voxel v holds the kept points seg_points[seg_start[v]:seg_start[v + 1]],
    ascending."""

    def __init__(self, n, device):
        buf = torch.empty((9 * n + 3,), dtype=I32, device=device)      # one allocation, views below
        self.n = n
        self.counts = buf[0:2]
        at = 2
        for name, size in (("point_idx", n), ("unq_inv", n), ("unq_cnt", n), ("seg_points", n), ("seg_start", n + 1),
                           ("voxel_coords", 4 * n)):
            setattr(self, name, buf[at:at + size])
            at += size
        self.voxel_coords = self.voxel_coords.view(n, 4)
        if n == 0:
            buf.zero_()


def _points_ok(points, name="points", min_cols=4):
    _chk(points, name, F32)
    if points.dim() != 2 or points.shape[1] < min_cols:
        raise ValueError("%s must be (n, >= %d) float32, got %s" % (name, min_cols, tuple(points.shape)))


def dynamic_voxel_index(points, spec, batch_size, pillars):
    """points (n, 1 + C) float32 on the device, the reference's collated [batch_idx, x, y, z, ...] rows (scenes in any
    order) -> DynVoxelIndex.  pillars: cells in x and y only, z is not tested.  A row joins nothing when a cell lies outside
    the grid, a coordinate is NaN or its batch index lies outside [0, batch_size).  No host read."""
    pillars = int(bool(pillars))
    keys = spec.key_range(batch_size, pillars)
    if batch_size < 1 or keys >= 2 ** 31:
        raise ValueError("batch %d x grid %s gives %d keys: the reference's int32 merge_coords holds fewer than 2^31"
                         % (batch_size, spec.grid.tolist(), keys))
    _points_ok(points)
    n = points.shape[0]
    out = DynVoxelIndex(n, points.device)
    if n == 0:
        return out
    ws = workspace("pda_dyn_voxel_workspace_bytes", (n, max(1, (keys - 1).bit_length())),
                   "%d rows / %d keys out of range" % (n, keys), points.device)
    _call("pda_dyn_voxel_index", points, points.data_ptr(), n, points.shape[1], spec.range_c, spec.vsize_c, spec.grid_c,
          int(batch_size), pillars, out.counts.data_ptr(), out.point_idx.data_ptr(), out.unq_inv.data_ptr(),
          out.unq_cnt.data_ptr(), out.voxel_coords.data_ptr(), out.seg_start.data_ptr(), out.seg_points.data_ptr(),
          ws.data_ptr())
    return out


def scatter_mean(src, index, rows=None):
    """src (>= n_kept, C) float32, one row a kept point -> (rows, C): per voxel and column the float32 sum over the voxel's
    points in ascending point order divided by float32(count) -- torch_scatter.scatter_mean with the order of the sum
    fixed.  rows (default index.n) output rows; those beyond the voxel count are zero.  No backward."""
    _points_ok(src, "src", 1)
    rows = index.n if rows is None else int(rows)
    out = torch.empty((rows, src.shape[1]), dtype=F32, device=src.device)
    _call("pda_dyn_scatter_mean", src, src.data_ptr(), src.shape[1], index.seg_start.data_ptr(), index.seg_points.data_ptr(),
          index.counts.data_ptr(), rows, out.data_ptr())
    return out


class ScatterMax(torch.autograd.Function):
    """ScatterMax.apply(x, index, rows) -> (out, arg): x (>= n_kept, F) float32; out (rows, F) the maximum over a voxel's
    points, exact; arg (rows, F) int32 the lowest point row that attains it (torch_scatter's CPU rule: an update needs a
    strictly greater value).  The backward sends grad_out[v, f] to row arg[v, f] and writes every other entry as zero."""

    @staticmethod
    def forward(ctx, x, index, rows=None):
        _points_ok(x, "x", 1)
        rows = index.n if rows is None else int(rows)
        out = torch.empty((rows, x.shape[1]), dtype=F32, device=x.device)
        arg = torch.empty((rows, x.shape[1]), dtype=I32, device=x.device)
        _call("pda_dyn_scatter_max_fwd", x, x.data_ptr(), x.shape[1], index.seg_start.data_ptr(), index.seg_points.data_ptr(),
              index.counts.data_ptr(), rows, out.data_ptr(), arg.data_ptr())
        ctx.index, ctx.x_rows = index, x.shape[0]
        ctx.save_for_backward(arg)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, grad_out, _grad_arg):
        arg, = ctx.saved_tensors
        return scatter_max_backward(grad_out, arg, ctx.index, ctx.x_rows), None, None


def scatter_max_backward(grad_out, arg, index, x_rows, out=None):
    """grad_x (x_rows, F), every entry written by the kernel (out: a buffer to write into)."""
    grad_out = grad_out.contiguous()
    _chk(grad_out, "grad_out", F32)
    grad_x = torch.empty((x_rows, arg.shape[1]), dtype=F32, device=arg.device) if out is None else out
    _call("pda_dyn_scatter_max_bwd", arg, grad_out.data_ptr(), _chk(arg, "arg", I32), index.unq_inv.data_ptr(),
          index.counts.data_ptr(), x_rows, arg.shape[0], arg.shape[1], _chk(grad_x, "grad_x", F32))
    return grad_x


def pillar_feature_width(columns, use_absolute_xyz, with_distance):
    """Columns of a PFN input row for points of `columns` = 1 + C columns."""
    return (columns - 1 if use_absolute_xyz else columns - 4) + 6 + int(bool(with_distance))


class PillarFeatures(torch.autograd.Function):
    """PillarFeatures.apply(points, index, mean, spec, use_absolute_xyz, with_distance) -> (n, width): the rows
    DynamicPillarVFE feeds its first PFN layer, [points[:, 1:] or points[:, 4:], xyz - mean[unq_inv], xyz - cell centre,
    (|xyz|)], zero beyond n_kept.  Gradients reach the point features points[:, 4:] only: the coordinates are inputs."""

    @staticmethod
    def forward(ctx, points, index, mean, spec, use_absolute_xyz, with_distance):
        _points_ok(points)
        n, c1 = points.shape
        width = pillar_feature_width(c1, use_absolute_xyz, with_distance)
        out = torch.empty((n, width), dtype=F32, device=points.device)
        _call("pda_dyn_pillar_features", points, points.data_ptr(), n, c1, index.point_idx.data_ptr(),
              index.unq_inv.data_ptr(), index.voxel_coords.data_ptr(), _chk(mean, "mean", F32), index.counts.data_ptr(),
              spec.vsize_c, spec.offset_c, int(bool(use_absolute_xyz)), int(bool(with_distance)), out.data_ptr())
        ctx.index, ctx.shape, ctx.first = index, (n, c1), 3 if use_absolute_xyz else 0
        return out

    @staticmethod
    def backward(ctx, grad):
        n, c1 = ctx.shape
        g = grad.new_zeros((n, c1))
        if c1 > 4:
            # row i of grad belongs to point_idx[i]; rows beyond n_kept all name row 0 and must not reach it, so they go
            # to a spare row that is cut off
            rows = torch.arange(n, device=grad.device)
            dest = torch.where(rows < ctx.index.counts[0], ctx.index.point_idx.long(), torch.full_like(rows, n))
            spare = grad.new_zeros((n + 1, c1 - 4))
            spare[dest] = grad[:, ctx.first:ctx.first + c1 - 4]
            g[:, 4:] = spare[:n]
        return g, None, None, None, None, None


def collate_packed(pts, offsets):
    """The data stages' packed rows (n_total, C) + offsets (B + 1) int64 -> the reference's collated (n_total, 1 + C) rows
    [batch_idx, ...] without a host read: row i belongs to the scene b with offsets[b] <= i < offsets[b + 1] (empty scenes
    own no row)."""
    _chk(pts, "points", F32)
    _chk(offsets, "offsets", torch.int64)
    n = pts.shape[0]
    rows = torch.arange(n, dtype=torch.int64, device=pts.device)
    b = torch.searchsorted(offsets[1:].contiguous(), rows, right=True)
    out = torch.empty((n, pts.shape[1] + 1), dtype=F32, device=pts.device)
    out[:, 0] = b.to(F32)
    out[:, 1:] = pts
    return out
