#!/usr/bin/env python
"""Times the device KITTI evaluation (pdanet_amd/kitti_eval.py) on a synthetic KITTI-val-sized set: 3769 frames, Car /
Pedestrian / Cyclist, --gt GT (DontCare included) and up to --max-det detections a frame.  Prints one JSON line:
  device_ms     the three device stages and the sort on frames already on the device, plus the one read-back
                (CUDA events, median of --reps);
  end_to_end_ms get_official_eval_result from the lists of dicts: packing, the one upload, the stages, the read and the
                float64 composition (wall clock, median).
Run under rocprofv3 --kernel-trace --stats for the per-kernel split.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdanet_amd import kitti_eval as ke  # noqa: E402

CLS = ['Car', 'Pedestrian', 'Cyclist']
NAMES = CLS + ['Van', 'Person_sitting', 'DontCare']
DIMS = np.array([(3.9, 1.55, 1.6), (0.8, 1.75, 0.6), (1.75, 1.7, 0.6), (5.0, 2.1, 1.9), (0.8, 1.2, 0.6), (1, 1, 1)])


def synth(rng, n_frames, n_gt, max_det):
    gts, dts = [], []
    for _ in range(n_frames):
        cls = rng.choice(6, n_gt, p=[0.5, 0.15, 0.1, 0.05, 0.05, 0.15])
        loc = np.c_[rng.uniform(-20, 20, n_gt), rng.uniform(1.4, 1.9, n_gt), rng.uniform(5, 70, n_gt)].astype(np.float32)
        dims = DIMS[cls] * rng.uniform(0.9, 1.1, (n_gt, 3))
        x0, y0 = rng.uniform(0, 1100, n_gt), rng.uniform(100, 250, n_gt)
        bbox = np.c_[x0, y0, x0 + rng.uniform(15, 140, n_gt), y0 + rng.uniform(10, 120, n_gt)].astype(np.float32)
        gts.append({'name': np.array(NAMES)[cls], 'truncated': rng.choice([0.0, 0.2, 0.4, 0.8], n_gt),
                    'occluded': rng.integers(0, 4, n_gt).astype(np.float64), 'alpha': rng.uniform(-3, 3, n_gt),
                    'bbox': bbox, 'dimensions': dims, 'location': loc, 'rotation_y': rng.uniform(-np.pi, np.pi, n_gt)})
        hit = (rng.random(n_gt) < 0.8) & (cls < 3)
        m = int(hit.sum())
        n_fp = int(rng.integers(max_det // 2, max_det - m + 1))
        fx = rng.uniform(0, 1100, n_fp)
        dts.append({'name': np.concatenate([np.array(NAMES)[cls[hit]], np.array(CLS)[rng.integers(0, 3, n_fp)]]),
                    'alpha': rng.uniform(-3, 3, m + n_fp).astype(np.float32),
                    'bbox': np.concatenate([bbox[hit] + rng.normal(0, 3, (m, 4)),
                                            np.c_[fx, np.full(n_fp, 150.0), fx + 60, 150 + rng.uniform(10, 80, n_fp)]]
                                           ).astype(np.float32),
                    'dimensions': np.concatenate([dims[hit], DIMS[rng.integers(0, 3, n_fp)]]).astype(np.float32),
                    'location': np.concatenate([loc[hit] + rng.normal(0, 0.15, (m, 3)),
                                                np.c_[rng.uniform(-20, 20, n_fp), np.full(n_fp, 1.6),
                                                      rng.uniform(5, 70, n_fp)]]).astype(np.float32),
                    'rotation_y': rng.uniform(-np.pi, np.pi, m + n_fp).astype(np.float32),
                    'score': np.concatenate([rng.uniform(0.3, 1, m), rng.uniform(0, 0.7, n_fp)]).astype(np.float32)})
    return gts, dts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--gt", type=int, default=20)
    ap.add_argument("--max-det", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    gts, dts = synth(np.random.default_rng(a.seed), a.frames, a.gt, a.max_det)
    vocab = ke._vocab(CLS, *[ke._names(g) for g in gts], *[ke._names(d) for d in dts])
    plan = ke._Plan(CLS, list(vocab))
    fr = ke.frames_from_annos(gts, dts, vocab, torch.device('cuda'))
    ke._read(ke._run_stages(fr, plan, True)[2], plan)                  # warm-up
    dev = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        ke._read(ke._run_stages(fr, plan, True)[2], plan)
        e1.record()
        torch.cuda.synchronize()
        dev.append(e0.elapsed_time(e1))
    e2e = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result, ret = ke.get_official_eval_result(gts, dts, CLS)
        e2e.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"bench": "kitti_eval", "frames": a.frames, "gt_per_frame": a.gt, "max_det": a.max_det,
                      "pairs": fr.ov_total, "tasks": plan.T, "device_ms": round(float(np.median(dev)), 3),
                      "end_to_end_ms": round(float(np.median(e2e)), 1), "reps": a.reps,
                      "Car_3d_moderate_R40": round(float(ret['Car_3d/moderate_R40']), 4),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
