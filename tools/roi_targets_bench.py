#!/usr/bin/env python
"""Times the RoI target assignment of a two-stage training step on a synthetic batch: B = 4 scenes, M = 512 RoIs and T = 64
GT rows a scene (20-60 real), ROI_PER_IMAGE = 128, the PointRCNN thresholds, sampling by class.  Prints one JSON line per
variant with the median and the minimum over --reps batches (wall clock between two device synchronisations, which is what
a training step waits for) and the host synchronisations torch's sync debug mode reports for one batch:
  device      ProposalTargetLayer.forward (seeded, check=False): pda_roi_max_iou + pda_roi_sample_targets;
  loop        the reference-shaped per-scene loop on this repository's own boxes_iou3d_gpu and torch ops: the trimming
              loop, the per-class loop behind two .item() reads, three nonzero(), numpy / CPU-generator draws uploaded
              per scene, an advanced-indexing gather per output, then the labels and the canonical transformation.
--only device|loop runs one variant (for a `rocprofv3 --kernel-trace --stats` run of its own: kernel launches a batch =
calls / (warm-up + reps)).
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdanet_amd import box_utils, iou3d_nms_utils as iu  # noqa: E402
from pdanet_amd.proposal_target_layer import ProposalTargetLayer  # noqa: E402

CFG = {'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5, 'SAMPLE_ROI_BY_EACH_CLASS': True, 'CLS_SCORE_TYPE': 'cls', 'CLS_FG_THRESH': 0.6,
       'CLS_BG_THRESH': 0.45, 'CLS_BG_THRESH_LO': 0.1, 'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55}
DIMS = np.array([(3.9, 1.6, 1.56), (0.8, 0.6, 1.73), (1.76, 0.6, 1.73)])


def synth(rng, B, M, T):
    gt = np.zeros((B, T, 8), np.float32)
    rois = np.zeros((B, M, 7), np.float32)
    labels = np.ones((B, M), np.int64)
    for s in range(B):
        n = int(rng.integers(20, 61))
        cls = rng.integers(0, 3, n)
        g = np.zeros((n, 8))
        g[:, 0], g[:, 1], g[:, 2] = rng.uniform(0, 70, n), rng.uniform(-40, 40, n), rng.uniform(-1.5, -0.5, n)
        g[:, 3:6] = DIMS[cls] * rng.uniform(0.9, 1.1, (n, 3))
        g[:, 6], g[:, 7] = rng.uniform(-np.pi, np.pi, n), cls + 1
        gt[s, :n] = g
        src = rng.integers(0, n, M - 32)                                # 32 zero-padded rows, as proposal_layer leaves them
        scale = rng.choice([0.03, 0.1, 0.25, 0.6, 2.0], M - 32)[:, None]
        jit = g[src, :7] + rng.normal(0, 1, (M - 32, 7)) * scale * [1.5, 0.8, 0.2, 0.2, 0.1, 0.1, 0.2]
        rois[s, :M - 32] = jit
        labels[s, :M - 32] = g[src, 7]
    scores = rng.standard_normal((B, M)).astype(np.float32)
    return rois, scores, labels, gt


def loop_targets(rois, scores, labels, gt, cfg):
    """The reference's order of work, scene by scene (proposal_target_layer.py, roi_head_template.py:104-134)."""
    B, R = rois.shape[0], cfg['ROI_PER_IMAGE']
    out = {'rois': rois.new_zeros(B, R, 7), 'gt_of_rois': rois.new_zeros(B, R, 8), 'gt_iou_of_rois': rois.new_zeros(B, R),
           'roi_scores': rois.new_zeros(B, R), 'roi_labels': labels.new_zeros(B, R)}
    fg_quota = int(np.round(cfg['FG_RATIO'] * R))
    for s in range(B):
        g = gt[s]
        k = len(g) - 1
        while k > 0 and g[k].sum() == 0:
            k -= 1
        g = g[:k + 1]
        g_lab = g[:, -1].long()
        best, arg = rois.new_zeros(rois.shape[1]), labels.new_zeros(rois.shape[1])
        for c in range(g_lab.min().item(), g_lab.max().item() + 1):
            rm, gm = labels[s] == c, g_lab == c
            if rm.sum() > 0 and gm.sum() > 0:
                v, i = iu.boxes_iou3d_gpu(rois[s][rm], g[gm][:, :7]).max(dim=1)
                best[rm] = v
                arg[rm] = gm.nonzero().view(-1)[i]
        fg = (best >= min(cfg['REG_FG_THRESH'], cfg['CLS_FG_THRESH'])).nonzero().view(-1)
        easy = (best < cfg['CLS_BG_THRESH_LO']).nonzero().view(-1)
        hard = ((best < cfg['REG_FG_THRESH']) & (best >= cfg['CLS_BG_THRESH_LO'])).nonzero().view(-1)
        n_fg, n_bg = fg.numel(), hard.numel() + easy.numel()
        if n_fg > 0 and n_bg > 0:
            take = min(fg_quota, n_fg)
            fg = fg[torch.from_numpy(np.random.permutation(n_fg)).to(fg.device)[:take]]
            bg_this = R - take
        elif n_fg > 0:
            fg = fg[torch.from_numpy(np.floor(np.random.rand(R) * n_fg)).to(fg.device).long()]
            bg_this = 0
        else:
            fg, bg_this = fg[:0], R
        picks = [fg]
        if bg_this:
            if hard.numel() > 0 and easy.numel() > 0:
                n_hard = min(int(bg_this * cfg['HARD_BG_RATIO']), hard.numel())
            else:
                n_hard = bg_this if hard.numel() > 0 else 0
            if n_hard:
                picks.append(hard[torch.randint(0, hard.numel(), (n_hard,)).to(hard.device)])
            if bg_this - n_hard:
                picks.append(easy[torch.randint(0, easy.numel(), (bg_this - n_hard,)).to(easy.device)])
        sel = torch.cat(picks)
        out['rois'][s], out['roi_labels'][s], out['gt_iou_of_rois'][s] = rois[s][sel], labels[s][sel], best[sel]
        out['roi_scores'][s], out['gt_of_rois'][s] = scores[s][sel], g[arg[sel]]
    iou = out['gt_iou_of_rois']
    out['reg_valid_mask'] = (iou > cfg['REG_FG_THRESH']).long()
    cls = (iou > cfg['CLS_FG_THRESH']).long()
    cls[(iou > cfg['CLS_BG_THRESH']) & (iou < cfg['CLS_FG_THRESH'])] = -1
    out['rcnn_cls_labels'] = cls
    src = out['gt_of_rois']
    out['gt_of_rois_src'] = src.clone()
    ry = out['rois'][:, :, 6] % (2 * np.pi)
    can = src.clone()
    can[:, :, 0:3] -= out['rois'][:, :, 0:3]
    can[:, :, 6] -= ry
    can = box_utils.rotate_points_along_z(can.view(-1, 1, 8), -ry.view(-1)).view(B, -1, 8)
    h = can[:, :, 6] % (2 * np.pi)
    opp = (h > np.pi * 0.5) & (h < np.pi * 1.5)
    h[opp] = (h[opp] + np.pi) % (2 * np.pi)
    h[h > np.pi] -= 2 * np.pi
    can[:, :, 6] = h.clamp(-np.pi / 2, np.pi / 2)
    out['gt_of_rois'] = can
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def count_syncs(fn):
    """Host synchronisations of one call, as far as torch's sync debug mode sees them (with 'always' it warns at every
    occurrence; the mode's own notice that it is a prototype is not one of them)."""
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode(1)
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    return sum('called a synchronizing' in str(x.message) for x in w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rois", type=int, default=512)
    ap.add_argument("--max-gt", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", choices=["device", "loop"], default=None)
    a = ap.parse_args()
    np.random.seed(a.seed)
    torch.manual_seed(a.seed)
    rois, scores, labels, gt = (torch.from_numpy(x).cuda() for x in synth(np.random.default_rng(a.seed), a.batch, a.rois, a.max_gt))
    layer = ProposalTargetLayer(CFG)
    bd = {'batch_size': a.batch, 'rois': rois, 'roi_scores': scores, 'roi_labels': labels, 'gt_boxes': gt}
    seeds = iter(range(1, 1 << 30))
    variants = {'device': lambda: layer(bd, seed=next(seeds), check=False),
                'loop': lambda: loop_targets(rois, scores, labels, gt, CFG)}
    for name, fn in variants.items():
        if a.only and a.only != name:
            continue
        for _ in range(a.warmup):
            fn()
        ms = [timed(fn) for _ in range(a.reps)]
        syncs = None if a.only else count_syncs(fn)       # (kept out of a profiler run)
        print(json.dumps({"bench": "roi_targets", "variant": name, "batch": a.batch, "rois": a.rois, "max_gt": a.max_gt,
                          "roi_per_image": CFG['ROI_PER_IMAGE'], "ms_median": round(float(np.median(ms)), 4),
                          "ms_min": round(float(np.min(ms)), 4), "host_syncs_per_batch": syncs, "reps": a.reps,
                          "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
