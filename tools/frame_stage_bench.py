#!/usr/bin/env python
"""Times the frame preparation on the device (pdanet_amd.frame_stage, csrc/frame_stage.hip) against the numpy chains on the
same machine's host.

  * fov_filter on 4 raw KITTI-sized scans of 120 000 points: device inputs, check=False (the form a training loop uses),
    timed with device events over --windows windows of --iters calls after --warmup calls (the median window is
    reported, the spread next to it), and the same call captured once as a graph and replayed.  Host: calib.lidar_to_rect,
    calib.rect_to_img and get_fov_flag written with numpy, then points[flag], one scan after the other on one core.
  * the extraction of a KITTI-train-sized set, 3712 frames of 120 000 points and 8 boxes, in batches of --batch frames: the
    same device batch is extracted 3712 / batch times (count, the one host read of the total, write), timed end to end with
    a host clock around a final synchronise (extract_device_s), and again with every batch's scans copied from pageable
    host memory first (extract_with_upload_s).  Reading the scans from disk and writing the .bin files are not included on
    either side.  Host: the numpy statement of points_in_boxes_cpu and the shift, timed on --host-frames frames and scaled
    to 3712.
Prints one JSON line.  Needs a GPU.

    python tools/frame_stage_bench.py [--iters 100] [--windows 5] [--warmup 20] [--batch 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdanet_amd import frame_stage as fs  # noqa: E402

P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]], np.float32)
R0 = np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459],
               [0.007402527, 0.004351614, 0.9999631]], np.float32)
V2C = np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                [0.9998621, 0.00752379, 0.01480755, -0.2717806]], np.float32)
SHAPE = (375, 1242)
N_FRAMES = 3712


def scans(rng, B, n):
    ang, r = rng.uniform(-np.pi, np.pi, (B, n)), rng.uniform(1.0, 80.0, (B, n))
    return np.stack([r * np.cos(ang), r * np.sin(ang), rng.uniform(-3.0, 2.0, (B, n)), rng.uniform(0, 1, (B, n))], -1).astype(np.float32)


def numpy_fov(points):
    """kitti_dataset.py:407-413 with calibration_kitti.py's lidar_to_rect / rect_to_img."""
    one = np.ones((points.shape[0], 1), np.float32)
    rect = np.dot(np.hstack((points[:, 0:3], one)), np.dot(V2C.T, R0.T))
    hom = np.hstack((rect, one))
    h = np.dot(hom, P2.T)
    img = (h[:, 0:2].T / hom[:, 2]).T
    depth = h[:, 2] - P2.T[3, 2]
    flag = (img[:, 0] >= 0) & (img[:, 0] < SHAPE[1]) & (img[:, 1] >= 0) & (img[:, 1] < SHAPE[0]) & (depth >= 0)
    return points[flag]


def numpy_extract(points, boxes):
    """create_groundtruth_database's loop with the numpy statement of points_in_boxes_cpu (margin 1e-2)."""
    out = []
    m = np.float64(np.float32(1e-2))
    for b64 in boxes:
        cx, cy, cz, dx, dy, dz, rz = b64.astype(np.float32)
        zin = np.abs(points[:, 2] - cz).astype(np.float64) <= np.float64(dz) / 2.0
        cosa, sina = np.float32(np.cos(-np.float64(rz))), np.float32(np.sin(-np.float64(rz)))
        sx, sy = points[:, 0] - cx, points[:, 1] - cy
        lx, ly = sx * cosa + sy * (-sina), sx * sina + sy * cosa
        inside = zin & (np.abs(lx).astype(np.float64) < np.float64(dx) / 2.0 + m) & (np.abs(ly).astype(np.float64) < np.float64(dy) / 2.0 + m)
        p = points[inside]
        p[:, :3] -= b64[:3]
        out.append(p)
    return out


def windows(fn, iters, n_windows, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(n_windows):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "frame_stage_bench needs a GPU"
    rng = np.random.default_rng(0)
    n = 120000

    # ---- the FOV filter: 4 x 120 000 -----------------------------------------------------------------------------------------
    p = scans(rng, 4, n)
    packed = torch.from_numpy(p.reshape(-1, 4)).cuda()
    offs = torch.arange(0, 4 * n + 1, n, dtype=torch.int64, device="cuda")
    rows = np.tile(np.concatenate([P2.reshape(-1), R0.reshape(-1), V2C.reshape(-1)])[None], (4, 1)).astype(np.float32)
    cal = torch.from_numpy(fs.calib_records(rows)).cuda()
    shp = torch.tensor([SHAPE] * 4, dtype=torch.int32, device="cuda")

    def step():
        return fs.fov_filter((packed, offs, n), cal, shp, check=False)

    (_, out_offs, _), info = step()
    kept = info.cpu()[:, 1].tolist()
    fov_ms = windows(step, a.iters, a.windows, a.warmup)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    graph_ms = windows(g.replay, a.iters, a.windows, a.warmup)
    for b in range(4):
        numpy_fov(p[b])
    host = []
    for _ in range(a.host_iters):
        t0 = time.perf_counter()
        for b in range(4):
            numpy_fov(p[b])
        host.append((time.perf_counter() - t0) * 1e3)
    fov_np_ms = float(np.median(host))

    # ---- the extraction: 3712 frames x 120 000 points x 8 boxes, in batches -------------------------------------------------------
    B, m = a.batch, 8
    q = scans(rng, B, n)
    boxes = np.concatenate([rng.uniform(5, 60, (B * m, 1)), rng.uniform(-25, 25, (B * m, 1)), rng.uniform(-1.2, -0.6, (B * m, 1)),
                            np.tile([3.9, 1.6, 1.56], (B * m, 1)) * rng.uniform(0.8, 1.3, (B * m, 3)),
                            rng.uniform(-np.pi, np.pi, (B * m, 1))], 1)
    d_pts = torch.from_numpy(q.reshape(-1, 4)).cuda()
    d_offs = torch.arange(0, B * n + 1, n, dtype=torch.int64, device="cuda")
    d_boxes = torch.from_numpy(boxes.astype(np.float32)).cuda()
    d_boffs = torch.arange(0, B * m + 1, m, dtype=torch.int64, device="cuda")
    d_centre = torch.from_numpy(np.ascontiguousarray(boxes[:, :3])).cuda()
    n_batches = (N_FRAMES + B - 1) // B

    def extract_all():
        rows_out = 0
        for _ in range(n_batches):
            obj_points, _, _, _ = fs.gt_extract((d_pts, d_offs, n), d_boxes, d_boffs, d_centre, check=False)
            rows_out += obj_points.shape[0]
        torch.cuda.synchronize()
        return rows_out

    for _ in range(3):
        fs.gt_extract((d_pts, d_offs, n), d_boxes, d_boffs, d_centre, check=False)
    torch.cuda.synchronize()
    ext = []
    for _ in range(3):
        t0 = time.perf_counter()
        rows_out = extract_all()
        ext.append(time.perf_counter() - t0)
    # the same with every batch's scans uploaded from the host first (what a builder fed from disk pays)
    q_host = q.reshape(-1, 4)

    def extract_all_uploaded():
        for _ in range(n_batches):
            fs.gt_extract((torch.from_numpy(q_host).cuda(), d_offs, n), d_boxes, d_boffs, d_centre, check=False)
        torch.cuda.synchronize()

    up = []
    for _ in range(2):
        t0 = time.perf_counter()
        extract_all_uploaded()
        up.append(time.perf_counter() - t0)
    numpy_extract(q[0], boxes[:m])
    t0 = time.perf_counter()
    for f in range(a.host_frames):
        numpy_extract(q[f % B], boxes[(f % B) * m:(f % B + 1) * m])
    ext_np_s = (time.perf_counter() - t0) / a.host_frames * N_FRAMES
    print(json.dumps({
        "fov_scans": 4, "fov_points_per_scan": n, "fov_kept": kept,
        "fov_device_ms": round(fov_ms[0], 4), "fov_device_ms_min_max": [round(fov_ms[1], 4), round(fov_ms[2], 4)],
        "fov_graph_replay_ms": round(graph_ms[0], 4), "fov_graph_replay_ms_min_max": [round(graph_ms[1], 4), round(graph_ms[2], 4)],
        "fov_numpy_chain_ms": round(fov_np_ms, 3),
        "extract_frames": N_FRAMES, "extract_points_per_frame": n, "extract_boxes_per_frame": m, "extract_batch": B,
        "extract_rows": rows_out, "extract_device_s": round(float(np.median(ext)), 4),
        "extract_device_s_min_max": [round(min(ext), 4), round(max(ext), 4)],
        "extract_with_upload_s": round(min(up), 4), "extract_with_upload_s_runs": [round(x, 4) for x in up],
        "extract_numpy_s_scaled_from_frames": a.host_frames, "extract_numpy_s": round(ext_np_s, 2),
        "windows": a.windows, "iters": a.iters, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
