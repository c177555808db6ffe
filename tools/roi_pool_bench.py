#!/usr/bin/env python
"""Times the RoI pooling entries (csrc/roi_pool.hip), one device-event pair around every call, median and minimum of --iters
calls after --warmup calls; outputs are re-zeroed outside the timed span.

Part-A2-like shape: 128 rois x 16 384 points uniform in a 70 m x 80 m x 4 m slab, rois of car size centred on points, out 12,
max_pts_each_voxel 128, C = 128 and C = 4; roiaware_pool3d forward (collect + pool: two launches) and backward, max and avg.
PointRCNN-like shape: 4 scenes of 16 384 points, 128 boxes a scene enlarged by 1.0, 512 sampled points, C = 130;
roipoint_pool3d forward.  Each line carries the compulsory HBM bytes of the call (inputs once plus outputs once) and the
bandwidth they imply at the median.  Prints one JSON line per entry and variant.  Needs a GPU.

    python tools/roi_pool_bench.py [--iters 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdanet_amd import box_utils  # noqa: E402
from pdanet_amd.roiaware_pool3d_utils import roiaware_pool3d_cuda as aware  # noqa: E402
from pdanet_amd.roipoint_pool3d_utils import roipoint_pool3d_cuda as point  # noqa: E402


def timed(fn, reset, iters, warmup, nbytes):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for i in range(warmup + iters):
        reset()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    return {"median_ms": round(med, 4), "min_ms": round(float(np.min(ms)), 4), "calls": iters, "compulsory_bytes": int(nbytes),
            "implied_GBps": round(nbytes / med / 1e6, 1)}


def scene(rng, n):
    return np.stack([rng.uniform(0, 70, n), rng.uniform(-40, 40, n), rng.uniform(-3, 1, n)], 1).astype(np.float32)


def boxes_on(rng, pts, n):
    c = pts[rng.integers(0, len(pts), n)]
    size = np.array([3.9, 1.6, 1.56], np.float32) * rng.uniform(0.8, 1.2, (n, 3)).astype(np.float32)
    return np.concatenate([c, size, rng.uniform(-np.pi, np.pi, (n, 1)).astype(np.float32)], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "roi_pool_bench needs a GPU"
    dev = torch.device("cuda")
    name = torch.cuda.get_device_name(0)
    rng = np.random.default_rng(0)
    i32 = dict(dtype=torch.int32, device=dev)

    def emit(**line):
        line["device"] = name
        print(json.dumps(line), flush=True)

    # ---- Part-A2-like roiaware pooling ---------------------------------------------------------------------------------
    N, P, out, K = 128, 16384, 12, 128
    pts_np = scene(rng, P)
    rois, pts = torch.from_numpy(boxes_on(rng, pts_np, N)).to(dev), torch.from_numpy(pts_np).to(dev)
    V = out ** 3
    for C in (128, 4):
        feat = torch.from_numpy(rng.normal(size=(P, C)).astype(np.float32)).to(dev)
        am, sl = torch.zeros((N, out, out, out, C), **i32), torch.zeros((N, out, out, out, K), **i32)
        pf = torch.zeros((N, out, out, out, C), device=dev)
        g_out = torch.from_numpy(rng.normal(size=(N, out, out, out, C)).astype(np.float32)).to(dev)
        g_in = torch.zeros((P, C), device=dev)
        shape = {"rois": N, "points": P, "out": out, "max_pts_each_voxel": K, "channels": C}

        def reset():
            am.zero_(); sl.zero_(); pf.zero_()
        for method, tag in ((0, "max"), (1, "avg")):
            # inputs once (rois, points, features) + outputs once (slots, pooled features, and argmax for max)
            fwd_bytes = 4 * (N * 7 + P * 3 + P * C + N * V * K + N * V * C * (2 if method == 0 else 1))
            t = timed(lambda: aware.forward(rois, pts, feat, am, sl, pf, method), reset, a.iters, a.warmup, fwd_bytes)
            emit(entry="roiaware_pool3d_fwd", pool=tag, **shape, points_kept=int(sl[..., 0].sum()),
                 non_empty_voxels=int((sl[..., 0] > 0).sum()), **t)
            # max reads argmax and grad_out; avg reads the slots and grad_out; both write grad_in
            bwd_bytes = 4 * (N * V * C + (N * V * C if method == 0 else N * V * K) + P * C)
            t = timed(lambda: aware.backward(sl, am, g_out, g_in, method), g_in.zero_, a.iters, a.warmup, bwd_bytes)
            emit(entry="roiaware_pool3d_bwd", pool=tag, **shape, **t)
        del feat, am, sl, pf, g_out, g_in

    # ---- PointRCNN-like roipoint pooling -------------------------------------------------------------------------------
    B, M, S, C = 4, 128, 512, 130
    xyz_np = np.stack([scene(rng, P) for _ in range(B)])
    boxes_np = np.stack([boxes_on(rng, xyz_np[b], M) for b in range(B)])
    xyz = torch.from_numpy(xyz_np).to(dev)
    boxes = box_utils.enlarge_box3d(torch.from_numpy(boxes_np).to(dev).view(-1, 7), (1.0, 1.0, 1.0)).view(B, M, 7).contiguous()
    feat = torch.from_numpy(rng.normal(size=(B, P, C)).astype(np.float32)).to(dev)
    rows, flag = torch.zeros((B, M, S, 3 + C), device=dev), torch.zeros((B, M), **i32)

    def reset_rows():
        rows.zero_(); flag.zero_()
    nbytes = 4 * (B * P * 3 + B * M * 7 + B * P * C + B * M * S * (3 + C) + B * M)
    t = timed(lambda: point.forward(xyz, boxes, feat, rows, flag), reset_rows, a.iters, a.warmup, nbytes)
    emit(entry="roipoint_pool3d_fwd", scenes=B, points=P, boxes=M, sampled=S, channels=C, empty_boxes=int(flag.sum()), **t)


if __name__ == "__main__":
    main()
