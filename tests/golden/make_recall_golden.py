#!/usr/bin/env python
"""Generates tests/golden/recall.npz: the REFERENCE's recall bookkeeping (pcdet/models/detectors/detector3d_template.py
Detector3DTemplate.generate_recall_record) run on synthetic eval batches, called per scene exactly as its post_processing
calls it: box_preds = the scene's final boxes (the first num_pred rows of the padded boxes), the dict threaded through the
scenes of the batch.

detector3d_template.py is loaded with its package imports stubbed (reference_loader.py).  Its IoU is the reference's own
iou3d_nms_utils.boxes_iou3d_gpu on CPU tensors over the C oracle of the BEV overlap.  boxes_iou3d_gpu is wrapped to record
the matrix of each scene, whose max over the predictions is each kept GT row's max IoU (0 for a scene without predictions, NaN for a trimmed row).

Batches (pred (B, K, 7) float32 zero-padded, num_pred (B), gt (B, T, 8) or none, the threshold list):
  kitti16 / kitti64   B = 4, max_gt 16 / 64, up to 100 predictions: jittered from GT across IoU 0.1-0.95, false
                      positives, duplicates, headings near +-pi, touching boxes and boxes 1e-4 apart;
  once                B = 2, up to 500 predictions;
  exact               axis-aligned nested pairs with IoU exactly 0.5, identical boxes;
  thresh              a kitti-like batch with thresholds equal to recorded IoU values and float64 values that round to
                      them in float32 (a float64 comparison decides differently for the ones below);
  trim                zero rows in the middle, an all-zero scene, a trailing real row that sums to exactly 0 (values
                      whose partial sums are exact in every order), a scene without predictions;
  no_pred             every scene without predictions;  max_gt0   gt (B, 0, 8);  no_gt   no gt_boxes at all.

Run with the reference checkout:  python tests/golden/make_recall_golden.py /path/to/reference
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from reference_loader import DETECTOR_STUBS, cpu_torch, extension_stubs, load, reference_root  # noqa: E402

OUT = os.path.join(HERE, "recall.npz")
THRESH = [0.3, 0.5, 0.7]
DET = None                       # the reference's Detector3DTemplate, once load_reference has run
_LAST = []                       # the matrices its boxes_iou3d_gpu returned since the list was emptied


def load_reference(root):
    global DET
    cpu_torch()
    stubs = dict(DETECTOR_STUBS, **{"utils.common_utils": {}, "models.roi_heads": {}, "models.model_utils.model_nms_utils": {}})
    iou, det = load(root, "pcdet_ref", ["ops.iou3d_nms.iou3d_nms_utils", "models.detectors.detector3d_template"],
                    stubs=extension_stubs(stubs))
    real = iou.boxes_iou3d_gpu

    def recording_iou3d(a, b):
        r = real(a, b)
        _LAST.append(r)
        return r

    iou.boxes_iou3d_gpu = recording_iou3d
    DET = det.Detector3DTemplate


def run_reference(pred, num, gt, thresh):
    """Detector3DTemplate.post_processing's recall part over one batch -> (recall_dict, max_iou (B, T))."""
    B, T = pred.shape[0], (gt.shape[1] if gt is not None else 0)
    batch_dict = {'batch_size': B}
    if gt is not None:
        batch_dict['gt_boxes'] = torch.from_numpy(gt)
    max_iou = np.full((B, T), np.nan, np.float32)
    recall = {}
    for s in range(B):
        final_boxes = torch.from_numpy(pred[s, :num[s]])
        del _LAST[:]
        recall = DET.generate_recall_record(box_preds=final_boxes, recall_dict=recall, batch_index=s, data_dict=batch_dict,
                                            thresh_list=thresh)
        if gt is None:
            continue
        k = T - 1                                        # the rows it kept, as it trims them
        while k > 0 and torch.from_numpy(gt[s, k]).sum() == 0:
            k -= 1
        kept = k + 1 if T > 0 else 0
        if kept and num[s] > 0:
            assert len(_LAST) == 1 and _LAST[0].shape == (num[s], kept)
            max_iou[s, :kept] = _LAST[0].max(dim=0)[0].numpy()
        elif kept:
            max_iou[s, :kept] = 0
    return recall, max_iou


# ---- scenes ------------------------------------------------------------------------------------------------------------
DIMS = np.array([(3.9, 1.6, 1.56), (0.8, 0.6, 1.73), (1.76, 0.6, 1.73), (10.0, 2.9, 3.2)])


def _gt_rows(rng, n, span):
    cls = rng.integers(0, 3, n)
    g = np.zeros((n, 8), np.float32)
    g[:, 0] = rng.uniform(-span, span, n)
    g[:, 1] = rng.uniform(-span, span, n)
    g[:, 2] = rng.uniform(-1.8, -0.5, n)
    g[:, 3:6] = DIMS[cls] * rng.uniform(0.85, 1.15, (n, 3))
    g[:, 6] = rng.uniform(-np.pi, np.pi, n)
    g[:, 7] = cls + 1
    flip = rng.random(n) < 0.15                         # headings next to +-pi
    g[flip, 6] = np.where(rng.random(flip.sum()) < 0.5, np.pi, -np.pi) - np.sign(rng.standard_normal(flip.sum())) * 1e-4
    return g


def _jitter(rng, g, scale):
    p = g[:7].astype(np.float64).copy()
    p[0:2] += rng.normal(0, scale, 2) * g[3:5].mean()
    p[2] += rng.normal(0, scale) * g[5]
    p[3:6] *= np.exp(rng.normal(0, scale / 2, 3))
    p[6] += rng.normal(0, scale / 2)
    if rng.random() < 0.2:                              # the same box the other way round (heading +-pi)
        p[6] = p[6] + np.pi if p[6] < 0 else p[6] - np.pi
    return p.astype(np.float32)


def _scene_preds(rng, g, k_max, n_fp, span):
    rows = []
    for r in g:
        if rng.random() < 0.85:
            for _ in range(1 + (rng.random() < 0.3)):   # duplicates
                rows.append(_jitter(rng, r, rng.choice([0.02, 0.08, 0.15, 0.3, 0.6])))
    for _ in range(n_fp):                               # false positives
        fp = _gt_rows(rng, 1, span)[0, :7]
        rows.append(fp)
    if len(g) >= 2 and rng.random() < 0.5:              # touching and 1e-4 apart, along x of an axis-aligned copy
        t = g[0, :7].copy()
        t[6] = 0.0
        a = t.copy()
        a[0] = t[0] + t[3]
        b = t.copy()
        b[0] = np.float32(t[0] + t[3] + np.float32(1e-4))
        rows += [a, b]
        g[0, 6] = 0.0
    rows = np.array(rows, np.float32).reshape(-1, 7)[:k_max]
    return rows[rng.permutation(len(rows))]


def _batch(rng, B, max_gt, k_max, n_gt, n_fp, span):
    pred = np.zeros((B, k_max, 7), np.float32)
    num = np.zeros(B, np.int32)
    gt = np.zeros((B, max_gt, 8), np.float32)
    for s in range(B):
        m = int(rng.integers(n_gt[0], n_gt[1] + 1))
        g = _gt_rows(rng, m, span)
        p = _scene_preds(rng, g, k_max, int(rng.integers(n_fp[0], n_fp[1] + 1)), span)
        gt[s, :m] = g
        pred[s, :len(p)] = p
        num[s] = len(p)
    return pred, num, gt


def _exact_batch():
    """Axis-aligned: a 2.5 x 4 x 2 prediction strictly inside a 4 x 5 x 2 GT (BEV area 10 of 20, same heights): IoU
    20 / (20 + 40 - 20) = 0.5 exactly, and an identical copy of another GT."""
    gt = np.zeros((2, 4, 8), np.float32)
    pred = np.zeros((2, 8, 7), np.float32)
    gt[0, 0] = [10, 5, -1, 4, 5, 2, 0, 1]
    gt[0, 1] = [20, -5, -1, 3.5, 1.5, 1.5, 0.7, 1]
    gt[1, 0] = [-12, 8, -0.5, 4, 5, 2, 0, 2]
    gt[1, 1] = [30, 30, -1, 1.0, 0.5, 1.75, -2.5, 3]
    pred[0, 0] = [10, 5, -1, 2.5, 4, 2, 0]
    pred[0, 1] = gt[0, 1, :7]
    pred[1, 0] = [-12.5, 8.25, -0.5, 2.5, 4, 2, 0]
    pred[1, 1] = gt[1, 1, :7]
    return pred, np.array([2, 2], np.int32), gt


def _trim_batch(rng):
    B, T = 4, 8
    gt = np.zeros((B, T, 8), np.float32)
    for s in range(B):
        gt[s, :5] = _gt_rows(rng, 5, 30)
    gt[0, 2] = 0                                        # a zero row in the middle: kept and counted
    gt[0, 5:] = 0
    gt[1] = 0                                           # all rows zero: row 0 is kept, one GT that cannot be recalled
    zero_sum = np.array([2.0, -3.5, -1.0, 1.5, 0.5, 0.25, 0.25, 0.0], np.float32)
    assert zero_sum.sum() == 0
    gt[2, 5] = zero_sum                                 # trailing real row summing to 0: dropped
    gt[2, 3] = zero_sum                                 # the same in the middle: kept
    gt[3, 7] = gt[3, 0]                                 # last row real: everything kept
    pred, num, _ = _batch(rng, B, T, 40, (5, 5), (0, 6), 30)
    for s in range(B):                                  # re-derive the predictions from this batch's GT
        p = _scene_preds(rng, gt[s, :5].copy(), 40, 4, 30)
        pred[s] = 0
        pred[s, :len(p)] = p
        num[s] = len(p)
    num[3] = 0                                          # a scene without predictions
    pred[3] = 0
    return pred, num, gt


def _thresh_cases(max_iou):
    """Thresholds equal to recorded IoU values (float32), and float64 values that round to them: below by a quarter step
    (a float64 comparison would count the row, float32 does not) and above by a quarter step."""
    v = np.unique(max_iou[np.isfinite(max_iou) & (max_iou > 0.05) & (max_iou < 0.99)])
    pick = v[np.linspace(0, len(v) - 1, 4).astype(int)]
    out = []
    for x in pick:
        x32 = np.float32(x)
        step = float(np.spacing(x32))
        lo, hi = float(x32) - step / 4, float(x32) + step / 4
        assert np.float32(lo) == x32 and np.float32(hi) == x32 and lo < float(x32) < hi
        out += [float(x32), lo, hi]
    return out


def main():
    load_reference(reference_root())
    rng = np.random.default_rng(20261016)
    batches = []
    for i in range(3):
        batches.append(("kitti16",) + _batch(rng, 4, 16, 100, (3, 16), (5, 40), 35) + (THRESH,))
    for i in range(2):
        batches.append(("kitti64",) + _batch(rng, 4, 64, 100, (20, 45), (5, 30), 35) + (THRESH,))
    for i in range(2):
        batches.append(("once",) + _batch(rng, 2, 96, 500, (40, 96), (300, 480), 70) + (THRESH,))
    batches.append(("exact",) + _exact_batch() + ([0.3, 0.5, 0.7, 0.99],))
    batches.append(("trim",) + _trim_batch(rng) + (THRESH,))
    p, n, g = _batch(rng, 4, 16, 100, (3, 16), (5, 40), 35)
    _, mi = run_reference(p, n, g, THRESH)
    batches.append(("thresh", p, n, g, _thresh_cases(mi)))
    p, n, g = _batch(rng, 4, 16, 100, (3, 16), (5, 40), 35)
    batches.append(("no_pred", np.zeros_like(p), np.zeros_like(n), g, THRESH))
    batches.append(("max_gt0", p, n, np.zeros((4, 0, 8), np.float32), THRESH))
    batches.append(("no_gt", p, n, None, THRESH))

    out = {'n_batches': np.int64(len(batches))}
    for i, (case, pred, num, gt, thresh) in enumerate(batches):
        recall, max_iou = run_reference(pred, num, gt, thresh)
        out['b%d_case' % i] = np.array(case)
        out['b%d_pred' % i] = pred
        out['b%d_num' % i] = num
        if gt is not None:
            out['b%d_gt' % i] = gt
        out['b%d_thresh' % i] = np.array(thresh, np.float64)
        out['b%d_recall_keys' % i] = np.array(list(recall.keys()), dtype='<U40')
        out['b%d_recall_vals' % i] = np.array([recall[k] for k in recall], np.int64)
        out['b%d_max_iou' % i] = max_iou
        print(case, pred.shape, None if gt is None else gt.shape, recall)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
