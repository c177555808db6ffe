#!/usr/bin/env python
"""Generates tests/golden/once_eval.npz: the REFERENCE's ONCE evaluation (pcdet/datasets/once/once_eval/evaluation.py,
eval_utils.py, iou_utils.py) run on ~30 synthetic ONCE-like frames.

numba is stubbed (reference_loader.stub_numba), and rotate_iou_gpu_eval is a loop over the reference's own
devRotateIoUEval(pred, gt, 2) with the same float32 casts and return dtype.  num_parts = the number of frames, so only per-frame blocks are computed (as the reference uses them).
get_thresholds and compute_statistics are wrapped to record the thresholds, num_valid_gt and summed tp / fp / fn of
every (class, difficulty).

The scenes hold all five classes and one unknown name, GT in float64 and predictions in float32, jittered true
positives, headings flipped near pi, duplicates, false positives, exact score ties, a frame without predictions, a
frame without GT, a class without GT (Bus) and one frame with more than 64 GT and 256 predictions.  Knife edges are
redrawn: |iou - thr| < 1e-3 for 0.3 / 0.5 / 0.7, distances within 1e-3 of 30 or 50, folded heading differences within
1e-3 of pi / 2 or pi, and any pair for which the stubbed reference overflows its 16-float point buffer.

Run with the reference checkout:  python tests/golden/make_once_eval_golden.py /path/to/reference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from reference_loader import load, reference_root, stub_numba  # noqa: E402

NAMES = ['Car', 'Bus', 'Truck', 'Pedestrian', 'Cyclist', 'Tricycle']
CLASSES = ['Car', 'Bus', 'Truck', 'Pedestrian', 'Cyclist']
DIMS = {'Car': (4.5, 1.9, 1.6), 'Bus': (11.0, 2.8, 3.2), 'Truck': (8.0, 2.6, 3.0), 'Pedestrian': (0.7, 0.7, 1.7),
        'Cyclist': (1.8, 0.8, 1.6), 'Tricycle': (2.6, 1.3, 1.6)}
THRS = (0.3, 0.5, 0.7)
CONFIGS = [
    ('default', {}),
    ('no_superclass', {'use_superclass': False}),
    ('overall', {'difficulty_mode': 'Overall'}),
    ('distance', {'difficulty_mode': 'Distance'}),
    ('no_heading', {'ap_with_heading': False}),
    ('pr40', {'num_pr_points': 40}),
]


REFM = {}                        # the reference's iou_utils, eval_utils and evaluation by name, once load_reference has run
_INTER = {}


def load_reference(root):
    stub_numba()
    names = ("iou_utils", "eval_utils", "evaluation")
    REFM.update(zip(names, load(root, "pcdet_ref", ["datasets.once.once_eval." + name for name in names])))
    REFM["evaluation"].rotate_iou_gpu_eval = rotate_iou_loop
    return REFM


def _pair_area(p5, g5):
    key = (p5.tobytes(), g5.tobytes())
    if key not in _INTER:
        _INTER[key] = REFM["iou_utils"].devRotateIoUEval(p5, g5, 2)
    return _INTER[key]


def rotate_iou_loop(boxes, query_boxes, criterion=-1, device_id=0):
    """rotate_iou_gpu_eval with its kernel body called per pair: dev_iou[n, k] = devRotateIoUEval(query_k, box_n)."""
    assert criterion == 2
    b32, q32 = boxes.astype(np.float32), query_boxes.astype(np.float32)
    iou = np.zeros((b32.shape[0], q32.shape[0]), np.float32)
    for n in range(b32.shape[0]):
        for k in range(q32.shape[0]):
            iou[n, k] = _pair_area(np.ascontiguousarray(q32[k]), np.ascontiguousarray(b32[n]))
    return iou.astype(boxes.dtype)


def ref_ious(gt_boxes, pred_boxes, heading):
    ev = REFM["evaluation"]
    return (ev.iou3d_kernel_with_heading if heading else ev.iou3d_kernel)(gt_boxes, pred_boxes)


def _dist_ok(b):
    d = float(np.sqrt(np.sum(b[0:3] * b[0:3])))
    return abs(d - 30) >= 1e-3 and abs(d - 50) >= 1e-3


def _fold(dh):
    dh = abs(dh)
    return 2 * np.pi - dh if dh >= np.pi else dh


def _pair_ok(g, p):
    try:
        v = ref_ious(g[None].astype(np.float64), p[None], False)[0, 0]
    except IndexError:                 # the stubbed point buffer overflowed (coincident edges)
        return False
    if not np.isfinite(v) or any(abs(v - t) < 1e-3 for t in THRS):
        return False
    f = _fold(float(g[6]) - float(np.float64(p[6])))
    return abs(f - np.pi / 2) >= 1e-3 and abs(f - np.pi) >= 1e-3


def _gt_box(rng, name):
    while True:
        r, a = rng.uniform(3, 75), rng.uniform(-np.pi, np.pi)
        l, w, h = (d * rng.uniform(0.85, 1.15) for d in DIMS[name])
        b = np.array([r * np.cos(a), r * np.sin(a), rng.normal(0, 0.4), l, w, h, rng.uniform(-np.pi, np.pi)])
        if _dist_ok(b):
            return b


def _pred_from(rng, g, flip):
    p = g.copy()
    p[0:2] += rng.normal(0, 0.1, 2)
    p[2] += rng.normal(0, 0.05)
    p[3:6] *= rng.uniform(0.93, 1.07, 3)
    p[6] += rng.normal(0, 0.05) + (np.pi if flip else 0)
    if p[6] > np.pi:
        p[6] -= 2 * np.pi
    return p.astype(np.float32)


def make_frame(rng, n_gt, n_fp, no_pred=False):
    gt_names = rng.choice(['Car', 'Car', 'Car', 'Truck', 'Pedestrian', 'Pedestrian', 'Cyclist', 'Tricycle'], n_gt)
    gt = np.array([_gt_box(rng, n) for n in gt_names]).reshape(-1, 7)
    if no_pred:
        return gt, gt_names, np.zeros((0, 7)), np.zeros(0), np.zeros(0)
    preds, names, scores = [], [], []
    ties = [0.5, 0.8, 0.25]

    def score():
        return np.float32(rng.choice(ties) if rng.random() < 0.25 else rng.uniform(0.05, 1.0))

    for i in range(n_gt):
        if rng.random() < 0.25:
            continue
        for _ in range(2 if rng.random() < 0.12 else 1):        # duplicates
            name = gt_names[i] if rng.random() < 0.85 else rng.choice(NAMES)
            preds.append((i, name, rng.random() < 0.1))
    for _ in range(n_fp):
        preds.append((-1, rng.choice(NAMES + ['Bus', 'Bus']), False))
    out_b, out_n, out_s = [], [], []
    for i, name, flip in preds:
        for _ in range(200):
            if i >= 0:
                p = _pred_from(rng, gt[i], flip)
            else:
                dname = name if name in DIMS else 'Car'
                p = _gt_box(rng, dname).astype(np.float32)
                if rng.random() < 0.5 and n_gt:               # near some GT: partial overlaps
                    p[0:2] = (gt[rng.integers(n_gt)][0:2] + rng.normal(0, 1.5, 2)).astype(np.float32)
            if _dist_ok(p.astype(np.float32)) and all(_pair_ok(g, p) for g in gt):
                break
        else:
            continue
        out_b.append(p)
        out_n.append(name)
        s = score()
        if out_s and rng.random() < 0.1:
            s = out_s[-1]                                      # exact tie with the previous prediction
        out_s.append(s)
    order = rng.permutation(len(out_b))
    pb = np.array(out_b, np.float32).reshape(-1, 7)[order]
    return gt, gt_names, pb, np.array(out_n)[order], np.array(out_s, np.float32)[order]


def build_scenes(seed=7):
    rng = np.random.default_rng(seed)
    frames = []
    for f in range(30):
        if f == 5:
            frames.append(make_frame(rng, 12, 6, no_pred=True))
        elif f == 9:
            frames.append(make_frame(rng, 0, 9))
        elif f == 17:
            frames.append(make_frame(rng, 70, 200))
        else:
            frames.append(make_frame(rng, int(rng.integers(3, 26)), int(rng.integers(0, 14))))
    gt_annos, pred_annos = [], []
    for gt, gn, pb, pn, ps in frames:
        gt_annos.append({'name': np.array(gn, dtype='<U10').reshape(-1), 'boxes_3d': np.array(gt, np.float64).reshape(-1, 7)})
        if len(pb) == 0:
            pred_annos.append({'name': np.zeros(0), 'score': np.zeros(0), 'boxes_3d': np.zeros((0, 7))})
        else:
            pred_annos.append({'name': np.array(pn), 'score': ps, 'boxes_3d': pb})
    return gt_annos, pred_annos


def run_reference(gt_annos, pred_annos, kwargs):
    ev = REFM["evaluation"]
    rec = []
    orig_thr, orig_stat = ev.get_thresholds, ev.compute_statistics

    def get_thresholds(scores, num_gt, num_pr_points):
        th = orig_thr(scores, num_gt, num_pr_points)
        rec.append({'thr': list(th), 'num_gt': int(num_gt), 'cm': np.zeros((len(th), 3), np.int64), 'k': 0})
        return th

    def compute_statistics(iou, pred_scores, gt_flag, pred_flag, score_threshold, iou_threshold):
        tp, fp, fn = orig_stat(iou, pred_scores, gt_flag, pred_flag, score_threshold, iou_threshold)
        r = rec[-1]
        t = r['k'] % len(r['thr'])
        assert r['thr'][t] == score_threshold
        r['cm'][t] += (tp, fp, fn)
        r['k'] += 1
        return tp, fp, fn

    ev.get_thresholds, ev.compute_statistics = get_thresholds, compute_statistics
    try:
        ret_str, ret_dict = ev.get_evaluation_results([dict(a) for a in gt_annos], [dict(a) for a in pred_annos],
                                                      list(CLASSES), num_parts=len(gt_annos), **kwargs)
    finally:
        ev.get_thresholds, ev.compute_statistics = orig_thr, orig_stat
    return ret_str, ret_dict, rec


def main():
    load_reference(reference_root())
    gt_annos, pred_annos = build_scenes()
    n_gt = np.array([len(a['name']) for a in gt_annos])
    n_pred = np.array([len(a['name']) for a in pred_annos])
    print("frames %d, GT %d, predictions %d, largest frame %d x %d" % (len(gt_annos), n_gt.sum(), n_pred.sum(),
                                                                      n_gt.max(), n_pred.max()))
    out = {
        'names': np.array(NAMES), 'classes': np.array(CLASSES),
        'gt_boxes': np.concatenate([a['boxes_3d'] for a in gt_annos]).astype(np.float64),
        'gt_name': np.concatenate([[NAMES.index(n) for n in a['name']] for a in gt_annos]).astype(np.int32),
        'gt_count': n_gt.astype(np.int64),
        'pred_boxes': np.concatenate([a['boxes_3d'] for a in pred_annos]).astype(np.float32),
        'pred_score': np.concatenate([a['score'] for a in pred_annos]).astype(np.float32),
        'pred_name': np.concatenate([[NAMES.index(n) for n in a['name']] for a in pred_annos]).astype(np.int32),
        'pred_count': n_pred.astype(np.int64),
    }
    for heading in (True, False):
        blocks = [ref_ious(g['boxes_3d'], p['boxes_3d'], heading).reshape(-1) for g, p in zip(gt_annos, pred_annos)]
        out['iou_heading' if heading else 'iou_plain'] = np.concatenate(blocks).astype(np.float64)
    for cname, kwargs in CONFIGS:
        ret_str, ret_dict, rec = run_reference(gt_annos, pred_annos, kwargs)
        P = kwargs.get('num_pr_points', 50)
        T = len(rec)
        thr = np.zeros((T, P + 1), np.float64)
        cm = np.zeros((T, P + 1, 3), np.int64)
        nthr = np.zeros(T, np.int64)
        for t, r in enumerate(rec):
            nthr[t] = len(r['thr'])
            thr[t, :nthr[t]] = r['thr']
            cm[t, :nthr[t]] = r['cm']
        out[cname + '/thresholds'] = thr
        out[cname + '/n_thresholds'] = nthr
        out[cname + '/num_valid_gt'] = np.array([r['num_gt'] for r in rec], np.int64)
        out[cname + '/counts'] = cm
        out[cname + '/ret_str'] = np.array(ret_str)
        out[cname + '/keys'] = np.array(list(ret_dict))
        out[cname + '/values'] = np.array([float(v) for v in ret_dict.values()], np.float64)
        print(cname, ret_str)
    path = os.path.join(HERE, "once_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
