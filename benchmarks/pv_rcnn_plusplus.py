#!/usr/bin/env python
"""Times what PV-RCNN++ adds, at the sizes waymo_models/pv_rcnn_plusplus.yaml runs it: 2 scenes x 180 000 raw points, 128 RoIs
per scene in training and 100 in test, NUM_KEYPOINTS 4 096, 6 sectors, the yaml's three filtered sources (raw points at 2.4 m,
2 x 60 000 x_conv3 voxel centres at 4.0 m, 2 x 25 000 x_conv4 voxel centres at 6.4 m).

sampling   keypoints (sample_points_with_roi + sector_fps) plus the three source filters, per RoI count:
             device    voxel_set_abstraction_spc.py: one pda_roi_point_filter launch per point set, a sort, one host read, one
                       stacked farthest-point-sampling launch; mask + nonzero + index_select per source
             composed  the same work as a torch composition in the reference's order on the same device: per scene and per
                       source an N x M distance matrix in parts of NUM_POINTS_OF_EACH_SAMPLE_PART (200 000) rows, a Python loop
                       over the sectors with an .item() in each, one stacked sampling launch per scene, boolean-mask gathers
           The composed side is the yardstick.  Masks and keypoints of the two sides are compared before anything is timed (the
           inputs are random: a point within float32 rounding of a threshold may differ, the count is reported).
interp     the rows of VectorPoolLocalInterpolateModule for x_conv3's two groups (C = 32, 27 cells, 2 x 4 096 keypoints) from a
           given three-NN result, forward + backward: pda_vector_interp_fwd / _bwd against the composed torch sequence
           (PDA_VECTOR_POOL); and the whole VectorPoolAggregationModuleMSG of x_conv3, forward + backward, on both paths.

The sides alternate inside one process; every figure is a device-event time over `--steps` calls (50 times as many for the
items of less than a millisecond: a filter alone, the interpolation rows) after `--warmup` calls, the median of `--repeats` windows, in milliseconds per call (the host reads of either side fall inside its window).  A measurement,
not a gate: prints one JSON line.

    python benchmarks/pv_rcnn_plusplus.py [--steps 10] [--warmup 3] [--repeats 5]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pdanet_amd import pointnet2_stack_utils, vector_pool_modules as vp             # noqa: E402
from pdanet_amd.config import to_attr                                               # noqa: E402
from pdanet_amd.voxel_set_abstraction_spc import sample_points_with_roi, sector_fps  # noqa: E402

PCR = [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0]
B, KEYPOINTS, SECTORS, PART = 2, 4096, 6, 200000
SHORT = 50              # the calls of less than a millisecond (a filter alone, the interpolation rows) get this many times the steps
SOURCES = {"raw_points": (180000, 2.4, 2), "x_conv3": (60000, 4.0, 64), "x_conv4": (25000, 6.4, 64)}   # rows per scene, radius, C
X_CONV3 = {'NAME': 'VectorPoolAggregationModuleMSG', 'NUM_GROUPS': 2, 'LOCAL_AGGREGATION_TYPE': 'local_interpolation',
           'NUM_REDUCED_CHANNELS': 32, 'NUM_CHANNELS_OF_LOCAL_AGGREGATION': 32, 'MSG_POST_MLPS': [128],
           'GROUP_CFG_0': {'NUM_LOCAL_VOXEL': [3, 3, 3], 'MAX_NEIGHBOR_DISTANCE': 1.2, 'NEIGHBOR_NSAMPLE': -1, 'POST_MLPS': [64, 64]},
           'GROUP_CFG_1': {'NUM_LOCAL_VOXEL': [3, 3, 3], 'MAX_NEIGHBOR_DISTANCE': 2.4, 'NEIGHBOR_NSAMPLE': -1, 'POST_MLPS': [64, 64]}}


def make_points(n, g):
    lo, hi = torch.tensor(PCR[:3], device="cuda"), torch.tensor(PCR[3:], device="cuda")
    return lo + (hi - lo) * torch.rand((B * n, 3), generator=g, device="cuda")


def make_rois(rois, g):
    """Vehicle-, pedestrian- and cyclist-sized boxes over the range, a tenth of them zero rows (the padding of the proposals)."""
    dims = torch.tensor([[4.7, 2.1, 1.7], [0.9, 0.85, 1.75], [1.8, 0.85, 1.75]], device="cuda")
    r = torch.zeros((B, rois, 7), device="cuda")
    u = lambda lo, hi: lo + (hi - lo) * torch.rand((B, rois), generator=g, device="cuda")
    r[..., 0], r[..., 1], r[..., 2] = u(-70, 70), u(-70, 70), u(-1, 2)
    r[..., 3:6] = dims[torch.randint(0, 3, (B, rois), generator=g, device="cuda")]
    r[..., 6] = u(-3.14159, 3.14159)
    r[torch.rand((B, rois), generator=g, device="cuda") < 0.1] = 0
    return r


# ---- the torch composition, in the reference's order of work ------------------------------------------------------------------
def composed_mask(rois, points, radius):
    """One scene: the N x M distances in parts of PART rows, the nearest RoI, its half diagonal."""
    parts = []
    for start in range(0, points.shape[0], PART):
        distance = (points[start:start + PART, None, :] - rois[None, :, 0:3]).norm(dim=-1)
        min_dis, nearest = distance.min(dim=-1)
        parts.append(min_dis < (rois[nearest, 3:6] / 2).norm(dim=-1) + radius)
    return torch.cat(parts) if parts else points.new_zeros((0,), dtype=torch.bool)


def composed_keypoints(rois, points, n_per_scene, radius):
    out = []
    for b in range(B):
        scene = points[b * n_per_scene:(b + 1) * n_per_scene]
        mask = composed_mask(rois[b], scene, radius)
        kept = scene[:1] if mask.sum() == 0 else scene[mask]
        sector = ((torch.atan2(kept[:, 1], kept[:, 0]) + math.pi) / (math.pi * 2 / SECTORS)).floor().clamp(min=0, max=SECTORS)
        chunks, counts, quotas = [], [], []
        for k in range(SECTORS):
            in_sector = sector == k
            n = in_sector.sum().item()
            if n > 0:
                chunks.append(kept[in_sector])
                counts.append(n)
                quotas.append(min(n, math.ceil(n / kept.shape[0] * KEYPOINTS)))
        xyz = torch.cat(chunks).contiguous()
        picked = pointnet2_stack_utils.stack_farthest_point_sample(xyz, torch.tensor(counts, device="cuda").int(), quotas).long()
        out.append(xyz[picked])
    return out


def composed_source(rois, xyz, feat, n_per_scene, radius):
    rows = torch.cat((xyz, feat), dim=-1)
    kept = []
    for b in range(B):
        scene = slice(b * n_per_scene, (b + 1) * n_per_scene)
        kept.append(rows[scene][composed_mask(rois[b], xyz[scene], radius)])
    return torch.cat(kept)


# ---- the device side ----------------------------------------------------------------------------------------------------------
def device_keypoints(rois, points, cnt, radius):
    mask, keys = sample_points_with_roi(rois, points, cnt, radius, num_sectors=SECTORS)
    rows, per_scene = sector_fps(points, mask, keys, B, KEYPOINTS, SECTORS)
    return points[rows], per_scene, mask


def device_source(rois, xyz, feat, cnt, radius):
    mask, _ = sample_points_with_roi(rois, xyz, cnt, radius)
    rows = torch.nonzero(mask).view(-1)
    return torch.cat((xyz.index_select(0, rows), feat.index_select(0, rows)), dim=-1)


def timed_alternating(fns, steps, warmup, repeats):
    """name -> [median, min, max] ms per call; the sides take turns, one window each, `repeats` times."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    windows = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            windows[k].append(t0.elapsed_time(t1) / steps)
    out = {}
    for k, w in windows.items():
        w.sort()
        out[k] = [round(w[len(w) // 2], 4), round(w[0], 4), round(w[-1], 4)]
    return out


def on_path(path, fn):
    def run():
        os.environ[vp.ENV] = path
        return fn()
    return run


def sampling_part(result, args, g):
    n_raw = SOURCES["raw_points"][0]
    sets = {}
    for name, (n, radius, c) in SOURCES.items():
        xyz = make_points(n, g)
        sets[name] = (xyz, torch.randn((B * n, c), generator=g, device="cuda"), torch.full((B,), n, dtype=torch.int32, device="cuda"),
                      n, radius)
    raw_xyz, raw_cnt = sets["raw_points"][0], sets["raw_points"][2]
    for tag, n_rois in (("train_2x128", 128), ("test_2x100", 100)):
        rois = make_rois(n_rois, g)

        def device():
            device_keypoints(rois, raw_xyz, raw_cnt, 1.6)
            for xyz, feat, cnt, n, radius in sets.values():
                device_source(rois, xyz, feat, cnt, radius)

        def composed():
            composed_keypoints(rois, raw_xyz, n_raw, 1.6)
            for xyz, feat, cnt, n, radius in sets.values():
                composed_source(rois, xyz, feat, n, radius)

        kp, per_scene, mask = device_keypoints(rois, raw_xyz, raw_cnt, 1.6)
        kp_ref = composed_keypoints(rois, raw_xyz, n_raw, 1.6)
        mask_ref = torch.cat([composed_mask(rois[b], raw_xyz[b * n_raw:(b + 1) * n_raw], 1.6) for b in range(B)])
        same_kp = [len(a) for a in kp_ref] == per_scene and torch.equal(torch.cat(kp_ref), kp)
        rows_kept = {k: int(device_source(rois, *v[:3], v[4]).shape[0]) for k, v in sets.items()}
        res = {"rois": [B, n_rois], "points_kept": int(mask.sum()), "mask_entries_that_differ": int((mask.bool() != mask_ref).sum()),
               "keypoints_per_scene": per_scene, "keypoints_equal": bool(same_kp), "source_rows_kept": rows_kept,
               "distance_matrix_megabytes_composed": round(n_raw * n_rois * 4 / 1e6, 1)}
        res.update(timed_alternating({"sampling_and_filters_device": device, "sampling_and_filters_composed": composed},
                                     args.steps, args.warmup, args.repeats))
        res.update(timed_alternating({"filter_raw_points_device": lambda: sample_points_with_roi(rois, raw_xyz, raw_cnt, 2.4),
                                      "filter_raw_points_composed": lambda: [composed_mask(rois[b], raw_xyz[b * n_raw:(b + 1) * n_raw], 2.4)
                                                                             for b in range(B)]},
                                     args.steps * SHORT, args.warmup, args.repeats))
        result[tag] = res


def interp_part(result, args, g):
    n, m, c = 20000, KEYPOINTS, 64                       # x_conv3 rows a filter leaves per scene, keypoints per scene
    xyz = make_points(n, g)
    xyz_cnt = torch.full((B,), n, dtype=torch.int32, device="cuda")
    new_xyz = xyz.view(B, n, 3)[:, :m].reshape(-1, 3).contiguous() + 0.05
    new_cnt = torch.full((B,), m, dtype=torch.int32, device="cuda")
    feat = torch.randn((B * n, c), generator=g, device="cuda").requires_grad_(True)
    torch.manual_seed(0)
    layer = vp.VectorPoolAggregationModuleMSG(input_channels=c, config=to_attr(X_CONV3)).cuda().train()
    res = {"support_rows": [B, n], "keypoints": [B, m], "channels": 32, "cells": 27}
    rows_of = {}
    for k, dist in ((0, 1.2), (1, 2.4)):
        group = getattr(layer, "layer_%d" % k)
        inner = group.local_interpolate_module
        centers = group.get_dense_voxels_by_center(new_xyz, dist, [3, 3, 3])
        reduced = feat.detach().view(B * n, -1, 32).sum(dim=1).requires_grad_(True)
        d, idx, _ = pointnet2_stack_utils.three_nn_for_vector_pool_by_two_step(xyz, xyz_cnt, new_xyz, centers, new_cnt, dist, -1, 0, 1000, 27, 2.0)
        grad = torch.randn((B * m * 27, 41), generator=g, device="cuda")

        def fused(reduced=reduced, d=d, idx=idx, centers=centers, grad=grad):
            reduced.grad = None
            vp.vector_interp(reduced, d, idx, xyz, centers).view(-1, 41).backward(grad)

        def composed(reduced=reduced, d=d, idx=idx, centers=centers, grad=grad, inner=inner):
            reduced.grad = None
            inner._rows_composed(xyz, reduced, centers, d, idx).backward(grad)

        a = vp.vector_interp(reduced, d, idx, xyz, centers).view(-1, 41)
        res["group_%d" % k] = {"max_neighbour_distance": dist, "cells_without_neighbour": int((idx[..., 0] < 0).sum()),
                               "output_megabytes": round(a.numel() * 4 / 1e6, 1),
                               "forward_bits_equal": bool(torch.equal(a, inner._rows_composed(xyz, reduced, centers, d, idx)))}
        rows_of["rows_fwd_bwd_fused_group_%d" % k], rows_of["rows_fwd_bwd_composed_group_%d" % k] = fused, composed

    def whole():
        layer.zero_grad(set_to_none=True)
        feat.grad = None
        layer(xyz=xyz, xyz_batch_cnt=xyz_cnt, new_xyz=new_xyz, new_xyz_batch_cnt=new_cnt, features=feat)[1].sum().backward()

    res.update(timed_alternating(rows_of, args.steps * SHORT, args.warmup, args.repeats))
    res.update(timed_alternating({"layer_fwd_bwd_fused": on_path("fused", whole), "layer_fwd_bwd_composed": on_path("composed", whole)},
                                 args.steps, args.warmup, args.repeats))
    os.environ.pop(vp.ENV, None)
    result["interp_x_conv3"] = res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/pv_rcnn_plusplus.py needs the GPU: a CPU run gives no time")
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    result = {"benchmark": "pv_rcnn_plusplus", "points": [B, SOURCES["raw_points"][0]], "keypoints": KEYPOINTS, "sectors": SECTORS,
              "steps": args.steps, "steps_of_short_items": args.steps * SHORT, "warmup": args.warmup, "repeats": args.repeats,
              "unit": "ms per call (median, min, max of the windows)"}
    sampling_part(result, args, g)
    interp_part(result, args, g)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
