#!/usr/bin/env python
"""Times the device ONCE evaluation (pdanet_amd/once_eval.py) on a synthetic ONCE-val-sized set: 3000 frames, 40 GT and
up to 500 predictions a frame (NMS_POST_MAXSIZE).  Prints one JSON line:
  device_ms     the three device stages and the sort on frames already on the device, plus the one read-back
                (CUDA events, median of --reps);
  end_to_end_ms get_evaluation_results from the lists of dicts: packing, the one upload, the stages, the read and the
                float64 AP composition (wall clock, median).
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
from pdanet_amd import once_eval as oe  # noqa: E402

CLS = ['Car', 'Bus', 'Truck', 'Pedestrian', 'Cyclist']
DIMS = np.array([(4.5, 1.9, 1.6), (11.0, 2.8, 3.2), (8.0, 2.6, 3.0), (0.7, 0.7, 1.7), (1.8, 0.8, 1.6)])


def synth(rng, n_frames, n_gt, max_pred):
    gts, preds = [], []
    for _ in range(n_frames):
        cls = rng.choice(5, n_gt, p=[0.5, 0.05, 0.1, 0.2, 0.15])
        r, a = rng.uniform(3, 75, n_gt), rng.uniform(-np.pi, np.pi, n_gt)
        boxes = np.c_[r * np.cos(a), r * np.sin(a), rng.normal(0, 0.3, n_gt), DIMS[cls] * rng.uniform(0.9, 1.1, (n_gt, 3)),
                      rng.uniform(-np.pi, np.pi, n_gt)]
        gts.append({'name': np.array(CLS)[cls], 'boxes_3d': boxes})
        hit = rng.random(n_gt) < 0.8
        tb = boxes[hit] + np.c_[rng.normal(0, 0.15, (hit.sum(), 3)), np.zeros((hit.sum(), 4))]
        n_fp = int(rng.integers(max_pred // 2, max_pred - hit.sum() + 1))
        fb = np.c_[rng.uniform(-75, 75, (n_fp, 2)), rng.normal(0, 0.5, n_fp), DIMS[rng.integers(0, 5, n_fp)],
                   rng.uniform(-np.pi, np.pi, n_fp)]
        preds.append({'name': np.concatenate([np.array(CLS)[cls[hit]], np.array(CLS)[rng.integers(0, 5, n_fp)]]),
                      'score': np.concatenate([rng.uniform(0.3, 1, hit.sum()), rng.uniform(0, 0.7, n_fp)]).astype(np.float32),
                      'boxes_3d': np.concatenate([tb, fb]).astype(np.float32)})
    return gts, preds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--gt", type=int, default=40)
    ap.add_argument("--max-pred", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    gts, preds = synth(np.random.default_rng(a.seed), a.frames, a.gt, a.max_pred)
    vocab = oe._vocab(CLS, *[oe._names(g) for g in gts], *[oe._names(p) for p in preds])
    plan = oe._Plan(CLS, list(vocab), True, None, 50, 'Overall&Distance')
    fr = oe.frames_from_annos(gts, preds, vocab, torch.device('cuda'))
    oe._read(oe._run_stages(fr, plan, True)[1], plan)                 # warm-up
    dev = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = oe._read(oe._run_stages(fr, plan, True)[1], plan)
        e1.record()
        torch.cuda.synchronize()
        dev.append(e0.elapsed_time(e1))
    e2e = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ret_str, ret = oe.get_evaluation_results(gts, preds, list(CLS))
        e2e.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"bench": "once_eval", "frames": a.frames, "gt_per_frame": a.gt, "max_pred": a.max_pred,
                      "pairs": fr.iou_total, "device_ms": round(float(np.median(dev)), 3),
                      "end_to_end_ms": round(float(np.median(e2e)), 1), "reps": a.reps,
                      "AP_mean_overall": round(float(ret['AP_mean/overall']), 4),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
