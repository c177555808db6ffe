#!/usr/bin/env python
"""Times the device augmentor (pdanet_amd.data_augmentor.DataAugmentor, csrc/augment.hip) followed by the device input
stage against a numpy statement of the same chain on the host, on 2 ONCE-like scenes of about 100k raw points and a
database of 300 objects (the ONCE yaml's SAMPLE_GROUPS, LIMIT_WHOLE_SCENE, flips on x and y, rotation, scaling).

Device: device inputs, check=False (no host read), the plan drawn on the host every call and uploaded, timed with device
events over --iters calls after --warmup calls: device_augment_ms (the augmentor alone) and device_augment_process_ms
(augmentor + DataProcessor to the collated 60000-point batch).  Host: numpy, one scene after the other on one core:
collision test of every candidate against the existing boxes and the other candidates (separating axes of the BEV
rectangles), the per-point box test of the pasted boxes (points_in_boxes_cpu's statement), the paste, the three world
transforms and limit_period -- numpy_augment_ms.  Prints one JSON line.  Needs a GPU.

    python tools/augment_bench.py [--iters 200] [--warmup 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdanet_amd import config, data_augmentor, data_processor  # noqa: E402

NAMES = ["Car", "Bus", "Truck", "Pedestrian", "Cyclist"]
DIMS = {"Car": (4.2, 1.8, 1.6), "Bus": (10.0, 2.8, 3.2), "Truck": (7.0, 2.5, 2.8), "Pedestrian": (0.7, 0.7, 1.7),
        "Cyclist": (1.8, 0.7, 1.5)}


def database(rng, n_db=300):
    boxes, points = {}, {}
    for n in NAMES:
        m = n_db // len(NAMES)
        d = np.array(DIMS[n]) * rng.uniform(0.9, 1.1, (m, 3))
        ctr = np.stack([rng.uniform(-60, 60, m), rng.uniform(-60, 60, m), -1.6 + d[:, 2] / 2], 1)
        boxes[n] = np.concatenate([ctr, d, rng.uniform(-np.pi, np.pi, (m, 1))], 1)
        points[n] = [np.concatenate([rng.uniform(-0.4, 0.4, (k, 3)) * d[i], rng.uniform(0, 1, (k, 1))], 1).astype(np.float32)
                     for i, k in enumerate(rng.integers(5, 300, m))]
    return boxes, points


def scenes(rng, n=100000, m=20):
    pts, bxs, cls = [], [], []
    for _ in range(2):
        r = np.sqrt(rng.uniform(1, 85 ** 2, n))
        a = rng.uniform(-np.pi, np.pi, n)
        pts.append(np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-2, 1, n), rng.uniform(0, 1, n)], 1).astype(np.float32))
        d = np.tile(DIMS["Car"], (m, 1))
        bxs.append(np.concatenate([rng.uniform(-70, 70, (m, 2)), np.full((m, 1), -0.8), d, rng.uniform(-3, 3, (m, 1))], 1)
                   .astype(np.float32))
        cls.append(rng.integers(0, 6, m).astype(np.int32))
    return pts, bxs, cls


def _corners2d(b):
    c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
    hx, hy = b[:, 3] / 2, b[:, 4] / 2
    sx, sy = np.array([1, 1, -1, -1]), np.array([1, -1, -1, 1])
    x = b[:, None, 0] + (sx * hx[:, None]) * c[:, None] - (sy * hy[:, None]) * s[:, None]
    y = b[:, None, 1] + (sx * hx[:, None]) * s[:, None] + (sy * hy[:, None]) * c[:, None]
    return np.stack([x, y], -1)                                        # (n, 4, 2)


def bev_overlap_np(a, b):
    """(na, nb) bool: the BEV rectangles overlap (no separating axis among the edge normals of either)."""
    ca, cb = _corners2d(a), _corners2d(b)
    sep = np.zeros((len(a), len(b)), bool)
    for e in range(2):
        ea = ca[:, e + 1] - ca[:, e]
        na = np.stack([-ea[:, 1], ea[:, 0]], -1)
        pa, pb = np.einsum('ikd,id->ik', ca, na), np.einsum('jkd,id->ijk', cb, na)
        sep |= (pa.max(-1)[:, None] < pb.min(-1)) | (pb.max(-1) < pa.min(-1)[:, None])
        eb = cb[:, e + 1] - cb[:, e]
        nb = np.stack([-eb[:, 1], eb[:, 0]], -1)
        pb, pa = np.einsum('jkd,jd->jk', cb, nb), np.einsum('ikd,jd->ijk', ca, nb)
        sep |= (pa.max(-1) < pb.min(-1)[None]) | (pb.max(-1)[None] < pa.min(-1))
    return ~sep


def points_in_boxes_np(p, boxes):
    out = np.zeros(len(p), bool)
    for b in boxes.astype(np.float32):
        zin = np.abs(p[:, 2] - b[2]) <= b[5] / 2
        c, s = np.float32(np.cos(-b[6])), np.float32(np.sin(-b[6]))
        sx, sy = p[:, 0] - b[0], p[:, 1] - b[1]
        lx, ly = sx * c + sy * (-s), sx * s + sy * c
        out |= zin & (np.abs(lx) < b[3] / 2 + 1e-2) & (np.abs(ly) < b[4] / 2 + 1e-2)
    return out


def numpy_augment(aug, db_boxes, db_points, pts_list, boxes_list, cls_list, plan):
    """gt_sampling + flip + rotation + scaling + limit_period, per scene on the host."""
    res = []
    for b, (p, bx, cl) in enumerate(zip(pts_list, boxes_list, cls_list)):
        ids, grp = plan['cand'][b], plan['cand_group'][b]
        existed = bx
        valid = []
        for g in np.unique(grp):
            sel = ids[grp == g]
            sb = db_boxes[sel].astype(np.float32)
            o2 = bev_overlap_np(sb, sb)
            np.fill_diagonal(o2, False)
            o1 = bev_overlap_np(sb, existed) if len(existed) else o2
            ok = ~(o1.any(1) | o2.any(1))
            valid.extend(sel[ok].tolist())
            existed = np.concatenate([existed, sb[ok]])
        vb = db_boxes[valid].astype(np.float32)
        obj = [db_points[i].copy() for i in valid]
        for o, i in zip(obj, valid):
            o[:, :3] += db_boxes[i, :3]
        p = p[~points_in_boxes_np(p, vb)]
        p = np.concatenate(obj + [p])
        bxo = np.concatenate([bx[cl > 0], vb])
        if plan['flip_x'][b]:
            p[:, 1] = -p[:, 1]; bxo[:, 1] = -bxo[:, 1]; bxo[:, 6] = -bxo[:, 6]
        if plan['flip_y'][b]:
            p[:, 0] = -p[:, 0]; bxo[:, 0] = -bxo[:, 0]; bxo[:, 6] = -(bxo[:, 6] + np.pi)
        a = plan['angle'][b]
        if a != 0:
            c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
            rot = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]], np.float32)
            p[:, :3] = p[:, :3] @ rot
            bxo[:, :3] = bxo[:, :3] @ rot
            bxo[:, 6] += a
        p[:, :3] *= plan['scale'][b]
        bxo[:, :6] *= plan['scale'][b]
        bxo[:, 6] = bxo[:, 6] - np.floor(bxo[:, 6] / np.float32(2 * np.pi) + np.float32(0.5)) * np.float32(2 * np.pi)
        res.append((p, bxo))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "augment_bench needs a GPU"
    cfg = config.load_yaml("once_pda_ssd.yaml")
    rng = np.random.default_rng(0)
    dbb, dbp = database(rng)
    db = data_augmentor.GtDatabase.from_arrays(NAMES, dbb, dbp)
    aug = data_augmentor.from_config(cfg, db)
    dp = data_processor.from_config(cfg, training=True)
    pts, boxes, cls = scenes(rng)
    n_cap = max(len(p) for p in pts)
    packed = torch.from_numpy(np.concatenate(pts)).cuda()
    offs = torch.tensor([0, len(pts[0]), len(pts[0]) + len(pts[1])], dtype=torch.int64, device="cuda")
    bx = torch.from_numpy(np.concatenate(boxes)).cuda()
    boffs = torch.tensor([0, len(boxes[0]), len(boxes[0]) + len(boxes[1])], dtype=torch.int64, device="cuda")
    torch.manual_seed(0)

    def step_aug():
        return aug((packed, offs, n_cap), (bx, boffs), cls, check=False)

    def step_all(i):
        pt, bt, _ = step_aug()
        return dp(pt, bt, max_gt=128, seed=i, check=False)

    def timed(fn):
        for i in range(a.warmup):
            fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.iters):
            fn(i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    aug_ms = timed(lambda i: step_aug())
    all_ms = timed(step_all)
    info = step_aug()[2].cpu().numpy()
    # host: the numpy statement on the same scenes with plans drawn the same way
    db_boxes = np.concatenate([dbb[n] for n in NAMES])
    db_points = [p for n in NAMES for p in dbp[n]]
    plans = [aug.make_plan(cls, np.random.default_rng(i)) for i in range(a.host_iters + 1)]
    numpy_augment(aug, db_boxes, db_points, pts, boxes, cls, plans[0])
    t0 = time.perf_counter()
    for i in range(a.host_iters):
        numpy_augment(aug, db_boxes, db_points, pts, boxes, cls, plans[i + 1])
    np_ms = (time.perf_counter() - t0) * 1e3 / a.host_iters
    print(json.dumps({"scenes": 2, "raw_points": [len(p) for p in pts], "db_objects": db.n_obj,
                      "candidates": [len(c) for c in plans[0]["cand"]], "accepted_last": info[:, 2].tolist(),
                      "points_out_last": info[:, 0].tolist(), "num_points": dp.num_points,
                      "device_augment_ms": round(aug_ms, 4), "device_augment_process_ms": round(all_ms, 4),
                      "numpy_augment_ms": round(np_ms, 3), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
