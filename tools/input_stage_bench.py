#!/usr/bin/env python
"""Times the device input stage (pdanet_amd.data_processor.DataProcessor, csrc/input_stage.hip) against the reference's
numpy chain on the host, on 2 ONCE-like scenes of about 100k raw points each sampled to 60000 (ONCE PDA-SSD.yaml).

Device: seeded mode, device inputs, fixed box capacity, no host read (the form a graphed training loop uses), timed with
device events over --iters calls after --warmup calls (device_stage_ms: calls from Python, back to back;
device_stage_graph_replay_ms: the same call captured once as a graph and replayed); host_lists_to_batch_ms: numpy lists
in, packing, the one transfer and the checked path's read included.  Host: the same chain written with numpy (range mask, depth split,
np.random.choice / shuffle / permutation, batch column, zero-padded boxes), one scene after the other on one core.
Prints one JSON line.  Needs a GPU.

    python tools/input_stage_bench.py [--iters 200] [--warmup 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdanet_amd import config, data_processor  # noqa: E402


def scenes(rng, n=100000, m=20):
    out, boxes = [], []
    for _ in range(2):
        r = np.sqrt(rng.uniform(1, 85 ** 2, n))
        a = rng.uniform(-np.pi, np.pi, n)
        p = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-2, 1, n), rng.uniform(0, 1, n)], 1).astype(np.float32)
        b = np.concatenate([rng.uniform(-70, 70, (m, 2)), np.full((m, 1), -1.0), np.tile([4.0, 1.8, 1.6], (m, 1)),
                            rng.uniform(-3, 3, (m, 1)), np.ones((m, 1))], 1).astype(np.float32)
        out.append(p)
        boxes.append(b)
    return out, boxes


def numpy_chain(pts_list, boxes_list, pcr, k):
    """mask_points_and_boxes_outside_range (points part + REMOVE_OUTSIDE_BOXES by corners) -> sample_points ->
    shuffle_points -> collate_batch, per scene on the host."""
    rows, kept = [], []
    tmpl = np.array([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]], np.float32) / 2
    for b, (p, bx) in enumerate(zip(pts_list, boxes_list)):
        p = p[(p[:, 0] >= pcr[0]) & (p[:, 0] <= pcr[3]) & (p[:, 1] >= pcr[1]) & (p[:, 1] <= pcr[4])]
        loc = bx[:, None, 3:6] * tmpl[None]
        c, s = np.cos(bx[:, 6])[:, None], np.sin(bx[:, 6])[:, None]
        cor = np.stack([loc[..., 0] * c - loc[..., 1] * s, loc[..., 0] * s + loc[..., 1] * c, loc[..., 2]], -1) + bx[:, None, :3]
        kept.append(bx[((cor >= pcr[:3]) & (cor <= pcr[3:])).all(-1).sum(1) >= 1])
        near = np.linalg.norm(p[:, :3], axis=1) < 40.0
        far_i, near_i = np.where(~near)[0], np.where(near)[0]
        if k < len(p):
            if k > len(far_i):
                choice = np.concatenate([np.random.choice(near_i, k - len(far_i), replace=False), far_i])
            else:
                choice = np.random.choice(np.arange(len(p)), k, replace=False)
        else:
            choice = np.concatenate([np.arange(len(p)), np.random.choice(np.arange(len(p)), k - len(p))])
        np.random.shuffle(choice)
        p = p[choice][np.random.permutation(k)]
        rows.append(np.pad(p, ((0, 0), (1, 0)), constant_values=b))
    gt = np.zeros((len(kept), max(len(x) for x in kept), kept[0].shape[1]), np.float32)
    for b, x in enumerate(kept):
        gt[b, :len(x)] = x
    return np.concatenate(rows), gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "input_stage_bench needs a GPU"
    cfg = config.load_yaml("once_pda_ssd.yaml")
    dp = data_processor.from_config(cfg, training=True)
    pcr = dp.point_cloud_range
    rng = np.random.default_rng(0)
    pts, boxes = scenes(rng)
    n_cap = max(len(p) for p in pts)
    packed = torch.from_numpy(np.concatenate(pts)).cuda()
    offs = torch.tensor([0, len(pts[0]), len(pts[0]) + len(pts[1])], dtype=torch.int64, device="cuda")
    bx = torch.from_numpy(np.concatenate(boxes)).cuda()
    boffs = torch.tensor([0, len(boxes[0]), len(boxes[0]) + len(boxes[1])], dtype=torch.int64, device="cuda")

    def step(i):
        return dp((packed, offs, n_cap), (bx, boffs), max_gt=64, seed=i, check=False)

    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(a.iters):
        step(i)
    e1.record()
    e1.synchronize()
    dev_ms = e0.elapsed_time(e1) / a.iters
    # the same call captured once and replayed: the device time of the five launches without the Python layer
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(0)
    for _ in range(a.warmup):
        g.replay()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.iters):
        g.replay()
    e1.record()
    e1.synchronize()
    graph_ms = e0.elapsed_time(e1) / a.iters
    # host inputs (numpy lists): packing + one transfer included, the check read included
    for i in range(3):
        dp(pts, boxes, max_gt=64, seed=i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.iters // 4):
        dp(pts, boxes, max_gt=64, seed=i)
    torch.cuda.synchronize()
    host_in_ms = (time.perf_counter() - t0) * 1e3 / (a.iters // 4)
    np.random.seed(0)
    numpy_chain(pts, boxes, pcr, dp.num_points)
    t0 = time.perf_counter()
    for _ in range(a.host_iters):
        numpy_chain(pts, boxes, pcr, dp.num_points)
    np_ms = (time.perf_counter() - t0) * 1e3 / a.host_iters
    print(json.dumps({"scenes": 2, "raw_points": [len(p) for p in pts], "num_points": dp.num_points,
                      "device_stage_ms": round(dev_ms, 4), "device_stage_graph_replay_ms": round(graph_ms, 4), "host_lists_to_batch_ms": round(host_in_ms, 4),
                      "numpy_chain_ms": round(np_ms, 3), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
