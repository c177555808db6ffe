"""Point-to-voxel on the device (csrc/voxel_stage.hip, include/pda_train.h pda_voxelize): the reference's
VoxelGeneratorWrapper (pcdet/datasets/processor/data_processor.py), i.e. the CPU path of spconv's point-to-voxel.

The contract is the loop in include/pda_train.h: cells from floor((p - lo) / voxel_size) in float32, voxels numbered in
order of first appearance, the first max_num_points_per_voxel points of a voxel kept in scene order, at most max_num_voxels
voxels.  spconv itself was not run against it.
"""
import ctypes

import numpy as np
import torch

from .pointnet2_batch_cuda import F32, _call, _chk
from .stage_common import workspace


def grid_size(point_cloud_range, voxel_size):
    """The cells along x, y, z as DataProcessor.sample_points_by_voxels computes them."""
    pr = np.asarray(point_cloud_range)
    return np.round((pr[3:6] - pr[0:3]) / np.array(voxel_size)).astype(np.int64)


def collate_voxels(voxels, coords, num_points, num_voxels):
    """The padded per-scene output of VoxelGenerator.generate_batch -> what the hard-voxel models take: voxels (V, P, C),
    voxel_coords (V, 4) int32 with the batch index in front (b, z, y, x), voxel_num_points (V) int32, scene after scene.
    One host read, of the B counts: the PFN layers' BatchNorm statistics must not see whole empty voxels, so the padding
    has to be cut off, and V depends on the data."""
    B, cap = num_points.shape
    counts = [min(max(int(v), 0), cap) for v in num_voxels.tolist()]      # the one host read; -1 marks unusable offsets
    vox = torch.cat([voxels[b, :n] for b, n in enumerate(counts)], dim=0)
    num = torch.cat([num_points[b, :n] for b, n in enumerate(counts)], dim=0)
    crd = torch.cat([torch.cat([coords.new_full((n, 1), b), coords[b, :n]], dim=1) for b, n in enumerate(counts)], dim=0)
    return vox.contiguous(), crd.contiguous(), num.contiguous()


def collate_voxels_padded(voxels, coords, num_points, num_voxels):
    """collate_voxels without the cut and without the host read: the same inputs -> voxels (B * max_voxels, P, C),
    voxel_coords (B * max_voxels, 4) int32, voxel_num_points (B * max_voxels) int32, num_active (1) int32, status (1) int32.
    The live rows come first, scene after scene, and equal collate_voxels' rows exactly (the counts clamped the same way);
    num_active is their number.  Dead rows: voxels 0, coordinates -1, num_points 0.  status is the zeroed flag word of the
    padded sparse tensors: the batch's voxel_num_active / voxel_status.
    A stable partition by index arithmetic (two scans and one indexed copy per tensor); nothing is read back."""
    _chk(voxels, "voxels", F32)
    _chk(coords, "coords", torch.int32)
    _chk(num_points, "num_points", torch.int32)
    _chk(num_voxels, "num_voxels", torch.int32)
    B, cap = num_points.shape
    dev = voxels.device
    rows = B * cap
    live = (torch.arange(cap, device=dev, dtype=torch.int32)[None, :] < num_voxels.clamp(0, cap)[:, None]).reshape(rows)
    before = live.cumsum(0)                                               # live rows up to and including this one
    total = before[-1:] if rows else before.new_zeros((1,))
    row = torch.arange(rows, device=dev)
    dest = torch.where(live, before - 1, total + (row - before))         # a permutation: the live rows first, both parts in order
    batch = torch.arange(B, device=dev, dtype=torch.int32)[:, None, None].expand(B, cap, 1)
    crd = torch.where(live[:, None], torch.cat([batch, coords], dim=2).reshape(rows, 4), coords.new_full((), -1))
    vox = torch.where(live[:, None, None], voxels.reshape((rows,) + tuple(voxels.shape[2:])), voxels.new_zeros(()))
    num = torch.where(live, num_points.reshape(rows), num_points.new_zeros(()))
    out = [torch.empty_like(t).index_copy_(0, dest, t) for t in (vox, crd, num)]
    return out[0], out[1], out[2], total.to(torch.int32), torch.zeros((1,), dtype=torch.int32, device=dev)


class VoxelSpec:
    """The host-side arguments of the voxel entries: range, voxel size and grid as C arrays."""

    def __init__(self, point_cloud_range, voxel_size, max_points, max_voxels):
        self.point_cloud_range = np.asarray(point_cloud_range, dtype=np.float32)
        self.voxel_size = np.asarray(voxel_size, dtype=np.float32)
        if self.point_cloud_range.shape != (6,) or self.voxel_size.shape != (3,):
            raise ValueError("point_cloud_range must hold 6 values and the voxel size 3")
        self.grid = grid_size(point_cloud_range, voxel_size)
        self.max_points, self.max_voxels = int(max_points), int(max_voxels)
        if self.max_points < 1 or self.max_voxels < 1:
            raise ValueError("MAX_POINTS_PER_VOXEL and MAX_NUMBER_OF_VOXELS must be positive")
        if (self.grid < 1).any() or (self.grid > 2 ** 31 - 1).any():
            raise ValueError("the voxel grid %s is empty or beyond int32" % (self.grid.tolist(),))
        self.range_c = (ctypes.c_float * 6)(*self.point_cloud_range.tolist())
        self.vsize_c = (ctypes.c_float * 3)(*self.voxel_size.tolist())
        self.grid_c = (ctypes.c_int32 * 3)(*self.grid.tolist())

    def workspace(self, batch, n_cap, max_points, dev):
        return workspace("pda_voxel_workspace_bytes", (batch, n_cap, self.max_voxels, max_points),
                         "batch %d / n_cap %d / max voxels %d / points per voxel %d out of range"
                         % (batch, n_cap, self.max_voxels, max_points), dev)


class VoxelGenerator:
    """VoxelGeneratorWrapper's signature.  generate(points) takes one scene; generate_batch takes packed scenes."""

    def __init__(self, vsize_xyz, coors_range_xyz, num_point_features, max_num_points_per_voxel, max_num_voxels):
        self.spec = VoxelSpec(coors_range_xyz, vsize_xyz, max_num_points_per_voxel, max_num_voxels)
        self.num_point_features = int(num_point_features)

    def generate_batch(self, points):
        """points: (packed (n_total, C) float32, offsets (B + 1) int64, n_cap), device tensors.  Returns voxels (B, max_voxels,
        max_points, C), coordinates (B, max_voxels, 3) int32 (z, y, x), num_points (B, max_voxels) int32 -- all zero beyond a
        scene's voxel count -- and num_voxels (B) int32 (-1: unusable offsets).  Nothing is read back."""
        pts, offs, n_cap = points
        sp = self.spec
        B, C, n_cap = offs.numel() - 1, pts.shape[1], max(int(n_cap), 1)
        if C != self.num_point_features:
            raise ValueError("points have %d columns, the generator was made for %d" % (C, self.num_point_features))
        dev = pts.device
        ws = sp.workspace(B, n_cap, sp.max_points, dev)
        voxels = torch.empty((B, sp.max_voxels, sp.max_points, C), dtype=torch.float32, device=dev)
        coords = torch.empty((B, sp.max_voxels, 3), dtype=torch.int32, device=dev)
        num_points = torch.empty((B, sp.max_voxels), dtype=torch.int32, device=dev)
        num_voxels = torch.empty((B,), dtype=torch.int32, device=dev)
        _call("pda_voxelize", pts, _chk(pts, "points", F32), _chk(offs, "offsets", torch.int64), pts.shape[0], B, C, n_cap,
              sp.range_c, sp.vsize_c, sp.grid_c, sp.max_voxels, sp.max_points, voxels.data_ptr(), coords.data_ptr(),
              num_points.data_ptr(), num_voxels.data_ptr(), ws.data_ptr())
        return voxels, coords, num_points, num_voxels

    def generate(self, points):
        """points (n, C), numpy or torch -> (voxels (V, max_points, C), coordinates (V, 3), num_points (V)) trimmed to the
        voxel count V (one host read): numpy arrays for a numpy input, device tensors otherwise."""
        as_numpy = not isinstance(points, torch.Tensor)
        pts = torch.as_tensor(np.asarray(points, np.float32) if as_numpy else points)
        pts = pts.to("cuda" if not pts.is_cuda else pts.device, torch.float32).contiguous()
        offs = torch.tensor([0, pts.shape[0]], dtype=torch.int64).to(pts.device)
        voxels, coords, num_points, num_voxels = self.generate_batch((pts, offs, pts.shape[0]))
        v = int(num_voxels.item())
        out = voxels[0, :v], coords[0, :v], num_points[0, :v]
        return tuple(t.cpu().numpy() for t in out) if as_numpy else out


def get_voxel_centers(voxel_coords, downsample_times, voxel_size, point_cloud_range):
    """common_utils.get_voxel_centers: voxel_coords (N, 3) [z, y, x] of a grid downsampled `downsample_times` -> centres
    (N, 3) [x, y, z] float32, in the reference's float32 expression."""
    assert voxel_coords.shape[1] == 3
    centers = voxel_coords[:, [2, 1, 0]].float()
    size = torch.tensor([float(v) for v in voxel_size], device=centers.device).float() * downsample_times
    lo = torch.tensor([float(v) for v in point_cloud_range[0:3]], device=centers.device).float()
    return (centers + 0.5) * size + lo


def generate_voxel2pinds(sparse_tensor):
    """common_utils.generate_voxel2pinds: (B, Z, Y, X) int32, the row of the active site in each cell and -1 elsewhere.
    A fill and one indexed store; nothing is read on the host."""
    ind = sparse_tensor.indices.long()
    rows = torch.arange(ind.shape[0], device=ind.device, dtype=torch.int32)
    out = torch.full([sparse_tensor.batch_size] + list(sparse_tensor.spatial_shape), -1, dtype=torch.int32, device=ind.device)
    out[ind[:, 0], ind[:, 1], ind[:, 2], ind[:, 3]] = rows
    return out
