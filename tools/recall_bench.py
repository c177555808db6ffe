#!/usr/bin/env python
"""Times the eval loop's 3-D recall bookkeeping on a synthetic KITTI-val-sized set: 3769 frames in batches of 4,
gt_boxes (4, 64, 8) with 1-64 real rows a frame, and --preds predictions a frame (50 and 500 = NMS_POST_MAXSIZE).  Prints
one JSON line per prediction count:
  device_ms     RecallRecorder.add over every batch plus compute() (the one read), CUDA events, median of --reps;
  reference_ms  generate_recall_record as the reference runs it, scene by scene, on this repository's boxes_iou3d_gpu:
                the trimming loop (a host read per row it looks at), one IoU matrix, and per threshold a max, a compare, a
                sum and an .item() (CUDA events around the whole loop, median of --ref-reps).
and one for the ONCE-size eval forward (2 x 16384 points, 64 GT rows a scene) with RECALL_MODE normal and speed (wall
clock of IASSD.forward under no_grad, which ends in a host read; the two modes interleaved, median of --fwd-reps).
Run under rocprofv3 --kernel-trace --stats with --quick for the per-kernel split (one rep each, no forward).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdanet_amd import iou3d_nms_utils as iu  # noqa: E402
from pdanet_amd.model_nms_utils import RecallRecorder  # noqa: E402

THRESH = [0.3, 0.5, 0.7]
DIMS = np.array([(3.9, 1.6, 1.56), (0.8, 0.6, 1.73), (1.76, 0.6, 1.73)])


def synth(rng, n_frames, max_gt, n_pred):
    n_gt = rng.integers(1, max_gt + 1, n_frames)
    gt = np.zeros((n_frames, max_gt, 8), np.float32)
    cls = rng.integers(0, 3, (n_frames, max_gt))
    real = np.arange(max_gt)[None, :] < n_gt[:, None]
    g = np.zeros((n_frames, max_gt, 8))
    g[..., 0], g[..., 1], g[..., 2] = rng.uniform(0, 70, g.shape[:2]), rng.uniform(-40, 40, g.shape[:2]), -1.0
    g[..., 3:6] = DIMS[cls] * rng.uniform(0.9, 1.1, g.shape[:2] + (3,))
    g[..., 6], g[..., 7] = rng.uniform(-np.pi, np.pi, g.shape[:2]), cls + 1
    gt[real] = g[real]
    pred = np.zeros((n_frames, n_pred, 7))                     # false positives everywhere, then 80 % of GT jittered
    pred[..., 0], pred[..., 1], pred[..., 2] = rng.uniform(0, 70, pred.shape[:2]), rng.uniform(-40, 40, pred.shape[:2]), -1.0
    pred[..., 3:6] = DIMS[rng.integers(0, 3, pred.shape[:2])]
    pred[..., 6] = rng.uniform(-np.pi, np.pi, pred.shape[:2])
    m = min(max_gt, n_pred)
    hit = real[:, :m] & (rng.random((n_frames, m)) < 0.8)
    jit = gt[:, :m, :7] + rng.normal(0, 0.2, (n_frames, m, 7)) * [1, 1, 0.2, 0.2, 0.1, 0.1, 0.2]
    pred[:, :m][hit] = jit[hit]
    return gt, pred.astype(np.float32), np.full(n_frames, n_pred, np.int32)


def reference_loop(gt_d, pred_scenes):
    """detector3d_template.py:288-329 per scene, the dict threaded through every scene of the set."""
    ret = {'gt': 0}
    for t in THRESH:
        ret['roi_%s' % str(t)] = 0
        ret['rcnn_%s' % str(t)] = 0
    for s, box in enumerate(pred_scenes):
        cur = gt_d[s]
        k = cur.__len__() - 1
        while k > 0 and cur[k].sum() == 0:
            k -= 1
        cur = cur[:k + 1]
        if cur.shape[0] > 0:
            iou = iu.boxes_iou3d_gpu(box[:, 0:7], cur[:, 0:7]) if box.shape[0] > 0 else None
            for t in THRESH:
                if iou is not None:
                    ret['rcnn_%s' % str(t)] += (iou.max(dim=0)[0] > t).sum().item()
            ret['gt'] += cur.shape[0]
    return ret


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def bench_set(a, n_pred):
    gt, pred, num = synth(np.random.default_rng(a.seed), a.frames, a.max_gt, n_pred)
    gt_d, pred_d, num_d = (torch.from_numpy(x).cuda() for x in (gt, pred, num))
    batches = [({'pred_boxes': pred_d[s:s + a.batch], 'num_pred': num_d[s:s + a.batch]}, gt_d[s:s + a.batch])
               for s in range(0, a.frames, a.batch)]
    rec = RecallRecorder(THRESH)

    def device_pass():
        rec.reset()
        for padded, g in batches:
            rec.add(padded, g)
        return rec.compute()

    device_pass()                                                        # warm-up
    dev = [timed(device_pass) for _ in range(a.reps)]
    metric, ret = dev[0][1]
    scenes = [pred_d[s, :int(num[s])] for s in range(a.frames)]
    reference_loop(gt_d[:8], scenes[:8])                                 # warm-up
    ref = [timed(lambda: reference_loop(gt_d, scenes)) for _ in range(a.ref_reps)]
    want = ref[0][1]
    match = metric['gt_num'] == want['gt'] and all(metric['recall_rcnn_%s' % t] == want['rcnn_%s' % t] for t in THRESH)
    dms, rms = float(np.median([d[0] for d in dev])), float(np.median([r[0] for r in ref]))
    return {"bench": "recall", "frames": a.frames, "batch": a.batch, "max_gt": a.max_gt, "preds_per_frame": n_pred,
            "batches": len(batches), "gt_num": metric['gt_num'], "device_ms": round(dms, 3),
            "device_us_per_batch": round(dms * 1e3 / len(batches), 2), "reference_ms": round(rms, 1),
            "reference_us_per_batch": round(rms * 1e3 / len(batches), 1), "speedup": round(rms / dms, 1),
            "match": bool(match), "recall_rcnn_0.7": round(ret['recall/rcnn_0.7'], 4), "reps": a.reps,
            "ref_reps": a.ref_reps, "device": torch.cuda.get_device_name(0)}


def bench_forward(a):
    from pdanet_amd import detector, synth as sy
    torch.manual_seed(0)
    model, cfg = detector.build_detector("once_pda_ssd.yaml")
    model = model.cuda().eval()
    B, N = 2, 16384
    pts = torch.from_numpy(sy.batch_points(B, N, config_id=2, dist="L")).cuda()
    gt, _, _ = synth(np.random.default_rng(a.seed + 1), B, 64, 1)
    gt[..., 0:2] -= [35.0, 0.0]
    bd = {'batch_size': B, 'points': pts, 'gt_boxes': torch.from_numpy(gt).cuda()}
    pp = model.model_cfg["POST_PROCESSING"]
    times = {'normal': [], 'speed': []}
    with torch.no_grad():
        for it in range(a.fwd_warmup + a.fwd_reps):
            for mode in ('normal', 'speed'):
                pp['RECALL_MODE'] = mode
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, rec = model(dict(bd))
                dt = (time.perf_counter() - t0) * 1e3
                assert (rec != {}) == (mode == 'normal')
                if it >= a.fwd_warmup:
                    times[mode].append(dt)
    pp['RECALL_MODE'] = 'normal'
    med = {m: float(np.median(v)) for m, v in times.items()}
    return {"bench": "recall_eval_forward", "config": "once_pda_ssd.yaml", "batch": B, "points": N, "max_gt": 64,
            "normal_ms": round(med['normal'], 3), "speed_ms": round(med['speed'], 3),
            "delta_ms": round(med['normal'] - med['speed'], 3),
            "normal_p10_p90": [round(float(np.percentile(times['normal'], q)), 3) for q in (10, 90)],
            "speed_p10_p90": [round(float(np.percentile(times['speed'], q)), 3) for q in (10, 90)],
            "reps": a.fwd_reps, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--max-gt", type=int, default=64)
    ap.add_argument("--preds", type=int, nargs="+", default=[50, 500])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-reps", type=int, default=1)
    ap.add_argument("--fwd-warmup", type=int, default=5)
    ap.add_argument("--fwd-reps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--quick", action="store_true", help="one rep of each set, no forward (for a profiler run)")
    a = ap.parse_args()
    if a.quick:
        a.reps, a.ref_reps = 1, 1
    for n_pred in a.preds:
        print(json.dumps(bench_set(a, n_pred)), flush=True)
    if not a.quick:
        print(json.dumps(bench_forward(a)), flush=True)


if __name__ == "__main__":
    main()
