"""Float64 restatements of what PV-RCNN++ adds (make_pv_rcnn_plusplus_golden.py, tests/test_pv_rcnn_plusplus.py): the RoI
filter and the sectors of sectorized proposal-centric sampling in numpy, the rows of VectorPoolLocalInterpolateModule in torch
(so that autograd gives the gradient of the support features).  Nothing here follows float32 rounding: where a decision of
the float32 run could differ, the generator's margins exclude the input."""
import math

import numpy as np
import torch


def roi_filter(points, rois, radius):
    """points (N, 3), rois (M, 7 + C) of ONE scene -> (margin, gap): margin[p] = distance to the nearest RoI centre minus that
    RoI's half diagonal minus radius (kept iff negative; the nearest is the lowest index among equals); gap[p] = the least
    difference between the nearest distance and the distance to a RoI with ANOTHER half diagonal (inf without one)."""
    p, r = np.asarray(points, np.float64), np.asarray(rois, np.float64)
    d = np.sqrt(((p[:, None, :] - r[None, :, 0:3]) ** 2).sum(-1))                  # (N, M)
    half = np.sqrt(((r[:, 3:6] / 2) ** 2).sum(-1))
    near = d.argmin(axis=1)                                                          # the first of equals
    d_near = d[np.arange(len(p)), near]
    other = half[None, :] != half[near][:, None]
    gap = np.where(other, d - d_near[:, None], np.inf).min(axis=1) if r.shape[0] else np.full(len(p), np.inf)
    return d_near - half[near] - radius, gap


def sector_position(points, num_sectors):
    """(atan2(y, x) + pi) / (2 pi / num_sectors): the sector is its floor, clamped to [0, num_sectors]."""
    p = np.asarray(points, np.float64)
    return (np.arctan2(p[:, 1], p[:, 0]) + np.pi) / (np.pi * 2 / num_sectors)


def sector_keys(scene, kept, position, num_sectors):
    sector = np.clip(np.floor(position), 0, num_sectors).astype(np.int64)
    return scene * (num_sectors + 1) + np.where(kept, sector, num_sectors)


def quotas(counts, kept, num_sampled_points):
    return [min(c, math.ceil(c / kept * num_sampled_points)) if c > 0 else 0 for c in counts]


def interp_rows(support_xyz, support_features, grid_centers, idx):
    """support_xyz (N, 3), support_features (N, C) [may require grad], grid_centers (M, G, 3), idx (M, G, 3) int with -1 in
    [..., 0] for a cell without neighbour -> (M, G * (C + 9)) float64."""
    xyz, feat, ctr = support_xyz.double(), support_features.double(), grid_centers.double()
    empty = idx[..., 0] < 0
    rows = idx.long().masked_fill(empty[..., None], 0)
    near = xyz[rows]                                                                 # (M, G, 3, 3)
    local = ctr[:, :, None, :] - near
    recip = 1.0 / (local.pow(2).sum(-1).sqrt() + 1e-8)
    weight = recip / recip.sum(-1, keepdim=True).clamp_min(1e-8)
    blend = (feat[rows] * weight[..., None]).sum(dim=2)                              # (M, G, C)
    out = torch.cat((blend, local.reshape(local.shape[0], local.shape[1], 9)), dim=-1).masked_fill(empty[..., None], 0)
    return out.reshape(out.shape[0], -1)


def interp_grad_out(rows, width):
    """The gradient the interpolation fixture is made with: a fixed pattern, not stored."""
    return np.cos(np.arange(rows * width, dtype=np.float64) * 0.37).astype(np.float32).reshape(rows, width)
