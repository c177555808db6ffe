#!/usr/bin/env python
"""Times the device voxel down-sampling chain (pdanet_amd.data_processor.DataProcessor with sample_points_by_voxels,
csrc/voxel_stage.hip + csrc/input_stage.hip) against the same chain on the host, on 2 and 8 Waymo-like sweeps of 180 000
points down-sampled to 65 536 (the DATA_PROCESSOR list of the reference's waymo_models/IA-SSD.yaml: range mask, shuffle,
VOXEL_SIZE [0.1, 0.1, 0.15], 5 points a voxel, 80 000 voxels, training mode).

Device: seeded mode, device inputs, no boxes, check=False (no host read), timed with device events over --iters calls after
--warmup calls (device_ms: calls from Python back to back; device_graph_replay_ms: the same call captured once and replayed).
Both are wall spans; the kernels' own time comes from running this tool with --device-only under a kernel trace.
Host: numpy_chain_ms = the chain vectorised with numpy (range mask, permutation, cells, np.unique for the first points,
sample_points, batch column), one scene after the other on one core; python_loop_ms = the point-by-point loop of the
CPU voxelizer written in plain Python, one scene, once, for reference (spconv's C++ loop was not available to time).
Prints one JSON line per batch size.  Needs a GPU.

    python tools/voxel_stage_bench.py [--iters 100] [--warmup 10] [--sample-type raw|mean_vfe] [--batches 2,8] [--device-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdanet_amd import data_processor  # noqa: E402

RANGE = [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0]
VOXEL_SIZE = [0.1, 0.1, 0.15]
MAX_POINTS, MAX_VOXELS, NUM_POINTS, C = 5, 80000, 65536, 5


def sweep(rng, n=180000):
    """A spinning-lidar-like sweep: areal density falling as 1 / r, most returns on the ground, some outside the range."""
    r = rng.uniform(1.5, 85.0, n)
    a = rng.uniform(-np.pi, np.pi, n)
    ground = rng.uniform(0, 1, n) < 0.65
    z = np.where(ground, -1.6 + rng.normal(0, 0.03, n), rng.uniform(-1.5, 3.5, n))
    p = np.stack([r * np.cos(a), r * np.sin(a), z, rng.uniform(0, 1, n), rng.uniform(0, 1, n)], 1).astype(np.float32)
    return p


def cfg(sample_type):
    return [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
            {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": True, "test": False}},
            {"NAME": "sample_points_by_voxels", "SAMPLE_TYPE": sample_type, "VOXEL_SIZE": VOXEL_SIZE,
             "MAX_POINTS_PER_VOXEL": MAX_POINTS, "MAX_NUMBER_OF_VOXELS": {"train": MAX_VOXELS, "test": 90000},
             "NUM_POINTS": {"train": NUM_POINTS, "test": NUM_POINTS}}]


def numpy_chain(pts_list, sample_type):
    pcr = np.array(RANGE, np.float32)
    lo, vs = pcr[:3], np.array(VOXEL_SIZE, np.float32)
    grid = np.round((pcr[3:6] - pcr[0:3]) / np.array(VOXEL_SIZE)).astype(np.int64)
    rows, n_vox = [], []
    for b, p in enumerate(pts_list):
        p = p[(p[:, 0] >= pcr[0]) & (p[:, 0] <= pcr[3]) & (p[:, 1] >= pcr[1]) & (p[:, 1] <= pcr[4])]
        p = p[np.random.permutation(len(p))]
        f = np.floor((p[:, :3] - lo) / vs)
        p, f = p[((f >= 0) & (f < grid)).all(1)], f[((f >= 0) & (f < grid)).all(1)]
        c = f.astype(np.int64)
        key = (c[:, 2] * grid[1] + c[:, 1]) * grid[0] + c[:, 0]
        uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
        order = np.argsort(first)[:MAX_VOXELS]
        if sample_type == "raw":
            v = p[first[order]]
        else:
            number = np.full(len(uniq), -1, np.int64)
            number[order] = np.arange(len(order))
            vox = number[inv.reshape(-1)]
            by = np.argsort(vox, kind="stable")
            rank = np.empty(len(vox), np.int64)
            rank[by] = np.arange(len(vox)) - np.searchsorted(vox[by], vox[by], side="left")
            put = (vox >= 0) & (rank < MAX_POINTS)
            voxels = np.zeros((len(order), MAX_POINTS, p.shape[1]), np.float32)
            voxels[vox[put], rank[put]] = p[put]
            v = voxels.sum(axis=1) / np.minimum(np.bincount(vox[vox >= 0], minlength=len(order)), MAX_POINTS)[:, None]
        n_vox.append(len(v))
        k = NUM_POINTS
        near = np.linalg.norm(v[:, :3], axis=1) < 40.0
        far_i, near_i = np.where(~near)[0], np.where(near)[0]
        if k < len(v):
            if k > len(far_i):
                choice = np.concatenate([np.random.choice(near_i, k - len(far_i), replace=False), far_i])
            else:
                choice = np.random.choice(np.arange(len(v)), k, replace=False)
        else:
            choice = np.concatenate([np.arange(len(v)), np.random.choice(np.arange(len(v)), k - len(v))])
        np.random.shuffle(choice)
        rows.append(np.pad(v[choice].astype(np.float32), ((0, 0), (1, 0)), constant_values=b))
    return np.concatenate(rows), n_vox


def python_loop(points):
    """The CPU voxelizer's loop, point by point (float32 through numpy scalars)."""
    pcr = np.array(RANGE, np.float32)
    lo, vs = pcr[:3], np.array(VOXEL_SIZE, np.float32)
    grid = np.round((pcr[3:6] - pcr[0:3]) / np.array(VOXEL_SIZE)).astype(np.int64).tolist()
    voxels = np.zeros((MAX_VOXELS, MAX_POINTS, points.shape[1]), np.float32)
    num = np.zeros(MAX_VOXELS, np.int32)
    index, voxel_num = {}, 0
    for i in range(points.shape[0]):
        cell = []
        for j in range(3):
            f = np.floor((points[i, j] - lo[j]) / vs[j])
            if not (f >= 0 and f < grid[j]):
                break
            cell.append(int(f))
        if len(cell) < 3:
            continue
        cell = tuple(cell)
        v = index.get(cell)
        if v is None:
            if voxel_num >= MAX_VOXELS:
                continue
            v = index[cell] = voxel_num
            voxel_num += 1
        if num[v] < MAX_POINTS:
            voxels[v, num[v]] = points[i]
            num[v] += 1
    return voxel_num


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--sample-type", default="raw", choices=["raw", "mean_vfe"])
    ap.add_argument("--device-only", action="store_true", help="skip the host chains and the graph (for a run under a kernel trace)")
    ap.add_argument("--batches", default="2,8", help="batch sizes, comma separated")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "voxel_stage_bench needs a GPU"
    dp = data_processor.DataProcessor(cfg(a.sample_type), RANGE, True, C)
    rng = np.random.default_rng(0)
    loop_ms = None
    for batch in [int(x) for x in a.batches.split(",")]:
        pts = [sweep(rng) for _ in range(batch)]
        n_cap = max(len(p) for p in pts)
        packed = torch.from_numpy(np.concatenate(pts)).cuda()
        offs = torch.tensor(np.concatenate([[0], np.cumsum([len(p) for p in pts])]), dtype=torch.int64, device="cuda")

        def step(i):
            return dp((packed, offs, n_cap), seed=i, check=False)

        for i in range(a.warmup):
            out = step(i)
        torch.cuda.synchronize()
        vinfo = out["voxel_info"].cpu().numpy()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.iters):
            step(i)
        e1.record()
        e1.synchronize()
        dev_ms = e0.elapsed_time(e1) / a.iters
        graph_ms = None
        if not a.device_only:
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
            graph_ms = round(e0.elapsed_time(e1) / a.iters, 4)
        line = {"scenes": batch, "raw_points": len(pts[0]), "num_points": NUM_POINTS, "sample_type": a.sample_type,
                "n_masked": vinfo[:, 0].tolist(), "n_voxels_before_cap": vinfo[:, 2].tolist(),
                "device_ms": round(dev_ms, 4), "device_graph_replay_ms": graph_ms}
        if not a.device_only:
            np.random.seed(0)
            numpy_chain(pts, a.sample_type)
            t0 = time.perf_counter()
            for _ in range(a.host_iters):
                _, n_vox = numpy_chain(pts, a.sample_type)
            line["numpy_chain_ms"] = round((time.perf_counter() - t0) * 1e3 / a.host_iters, 2)
            line["numpy_voxels"] = n_vox
            if loop_ms is None:
                t0 = time.perf_counter()
                python_loop(pts[0])
                loop_ms = (time.perf_counter() - t0) * 1e3
            line["python_loop_one_scene_ms"] = round(loop_ms, 1)
        line["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
