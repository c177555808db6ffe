"""Which of the cases tests/golden/roi_targets.npz has to contain it does contain: computed from the stored arrays alone, by
make_roi_targets_golden.py when it writes the fixture and by tests/test_roi_targets.py::test_fixture_covers_cases, so the
coverage cannot rot."""
import json

import numpy as np

REQUIRED = {
    'fg_bg_above_quota', 'fg_bg_below_quota', 'fg_only', 'bg_only', 'bg_both', 'bg_hard_only', 'bg_easy_only',
    'hard_below_quota', 'gt_zero_mid', 'gt_all_zero', 'gt_trailing_real', 'class_without_gt', 'noncontiguous_labels',
    'dup_gt', 'dup_gt_tie', 'zero_roi_rows', 'roi_heading_negative', 'roi_heading_above_2pi', 'roi_heading_near_pi',
    'fold_low', 'fold_mid', 'fold_high', 'overlap_shared', 'exact_ge', 'exact_gt', 'exact_lt', 'no_neither',
    'score_cls', 'score_roi_iou', 'by_class', 'agnostic', 'proposal_layout_3d', 'proposal_layout_batch_index',
    'proposal_more_columns_than_survivors', 'proposal_full',
}
SHAPES = {'B': {2, 3, 4}, 'M': {64, 128, 512}, 'T': {8, 16, 64}, 'R': {32, 128}}


def kept_rows(gt):
    """The reference's trimming of one scene's (T, 8) GT: the number of rows it keeps (never fewer than one)."""
    k = gt.shape[0] - 1
    while k > 0 and np.float32(gt[k].sum(dtype=np.float32)) == 0:
        k -= 1
    return k + 1


def category_counts(max_overlaps, cfg):
    """(fg, hard, easy) list lengths of one scene with the thresholds compared in float32, as torch compares them."""
    f = np.float32
    fg_t = f(min(cfg['REG_FG_THRESH'], cfg['CLS_FG_THRESH']))
    fg = max_overlaps >= fg_t
    easy = max_overlaps < f(cfg['CLS_BG_THRESH_LO'])
    hard = (max_overlaps < f(cfg['REG_FG_THRESH'])) & (max_overlaps >= f(cfg['CLS_BG_THRESH_LO']))
    return fg, hard, easy


def pick_counts(n_fg, n_hard, n_easy, cfg):
    """subsample_rois / sample_bg_inds on the list lengths -> (fg picks, hard picks, easy picks), None for neither."""
    R = int(cfg['ROI_PER_IMAGE'])
    quota = int(np.round(cfg['FG_RATIO'] * R))
    bg = n_hard + n_easy
    if n_fg > 0 and bg > 0:
        p_fg = min(quota, n_fg)
        bg_this = R - p_fg
    elif n_fg > 0:
        return R, 0, 0
    elif bg > 0:
        p_fg, bg_this = 0, R
    else:
        return None
    if n_hard > 0 and n_easy > 0:
        p_hard = min(int(bg_this * cfg['HARD_BG_RATIO']), n_hard)
    elif n_hard > 0:
        p_hard = bg_this
    else:
        p_hard = 0
    return p_fg, p_hard, bg_this - p_hard


def coverage(fx):
    """fx: the loaded npz (or the dict about to be saved) -> (set of covered case names, dict of the shapes seen)."""
    seen = set()
    shapes = {k: set() for k in SHAPES}
    two_pi, pi = np.float32(2 * np.pi), np.float32(np.pi)
    neither = False
    for i in range(int(fx['n_batches'])):
        p = 'b%d_' % i
        cfg = json.loads(str(fx[p + 'cfg']))
        rois, labels, gt, mo, ga = fx[p + 'rois'], fx[p + 'roi_labels'], fx[p + 'gt_boxes'], fx[p + 'max_overlaps'], fx[p + 'gt_assignment']
        B, M, T, R = rois.shape[0], rois.shape[1], gt.shape[1], int(cfg['ROI_PER_IMAGE'])
        for k, v in zip('BMTR', (B, M, T, R)):
            shapes[k].add(v)
        by_class = bool(cfg.get('SAMPLE_ROI_BY_EACH_CLASS', False))
        seen.add('by_class' if by_class else 'agnostic')
        seen.add('score_' + cfg['CLS_SCORE_TYPE'])
        quota = int(np.round(cfg['FG_RATIO'] * R))
        for s in range(B):
            fg, hard, easy = category_counts(mo[s], cfg)
            n_fg, n_hard, n_easy = int(fg.sum()), int(hard.sum()), int(easy.sum())
            picks = pick_counts(n_fg, n_hard, n_easy, cfg)
            if picks is None:
                neither = True
                continue
            if n_fg and n_hard + n_easy:
                seen.add('fg_bg_above_quota' if n_fg > quota else 'fg_bg_below_quota' if n_fg < quota else 'fg_bg_at_quota')
            elif n_fg:
                seen.add('fg_only')
            else:
                seen.add('bg_only')
            if n_hard + n_easy:
                seen.add('bg_both' if n_hard and n_easy else 'bg_hard_only' if n_hard else 'bg_easy_only')
                if n_hard and n_easy and n_hard < int((R - picks[0]) * cfg['HARD_BG_RATIO']):
                    seen.add('hard_below_quota')
            if (fg & hard).any():
                seen.add('overlap_shared')
            kept = kept_rows(gt[s])
            g = gt[s, :kept]
            zero = ~g.any(axis=1)
            if kept > 2 and zero[1:kept - 1].any():
                seen.add('gt_zero_mid')
            if kept == 1 and zero[0]:
                seen.add('gt_all_zero')
            if kept == T and not zero[T - 1]:
                seen.add('gt_trailing_real')
            gl = set(int(v) for v in g[~zero, 7])
            if by_class and (set(int(v) for v in labels[s]) - gl - {0}) and gl:
                seen.add('class_without_gt')
            if gl and set(range(min(gl), max(gl) + 1)) - gl:
                seen.add('noncontiguous_labels')
            for a in range(kept):
                for b in range(a + 1, kept):
                    if not zero[a] and (g[a] == g[b]).all():
                        seen.add('dup_gt')
                        if ((ga[s] == a) & (mo[s] > 0)).any():
                            seen.add('dup_gt_tie')      # a RoI overlapping both copies took the first
            if (~rois[s].any(axis=1)).any():
                seen.add('zero_roi_rows')
            ry = rois[s, :, 6]
            if (ry < 0).any():
                seen.add('roi_heading_negative')
            if (ry > two_pi).any():
                seen.add('roi_heading_above_2pi')
            if (np.abs(np.abs(ry) - pi) < 2e-4).any():
                seen.add('roi_heading_near_pi')
        # the fold branch of every sampled target, from the stored targets
        t_rois, t_src = fx[p + 't_rois'], fx[p + 't_gt_of_rois_src']
        roi_ry = np.mod(t_rois[..., 6], two_pi).astype(np.float32)
        h = np.mod((t_src[..., 6] - roi_ry).astype(np.float32), two_pi)
        if (h <= np.float32(np.pi * 0.5)).any():
            seen.add('fold_low')
        if ((h > np.float32(np.pi * 0.5)) & (h < np.float32(np.pi * 1.5))).any():
            seen.add('fold_mid')
        if (h >= np.float32(np.pi * 1.5)).any():
            seen.add('fold_high')
        if str(fx[p + 'case']).startswith('exact'):
            f = np.float32
            if (mo == f(min(cfg['REG_FG_THRESH'], cfg['CLS_FG_THRESH']))).any() and (mo == f(cfg['CLS_BG_THRESH_LO'])).any():
                seen.add('exact_ge')                    # fg >= and hard >= on equality
            ti = fx[p + 't_gt_iou_of_rois']
            if (ti == f(cfg['REG_FG_THRESH'])).any() and (ti == f(cfg['CLS_FG_THRESH'])).any() and (ti == f(cfg['CLS_BG_THRESH'])).any():
                seen.add('exact_gt')                    # reg_valid >, cls > and the ignore / interval bounds on equality
            if (mo == f(cfg['CLS_BG_THRESH_LO'])).any() and (mo == f(cfg['REG_FG_THRESH'])).any():
                seen.add('exact_lt')                    # easy < and hard < on equality
    if not neither:
        seen.add('no_neither')
    for i in range(int(fx['n_proposal'])):
        p = 'p%d_' % i
        cfg = json.loads(str(fx[p + 'nms_cfg']))
        seen.add('proposal_layout_' + str(fx[p + 'layout']))
        real = fx[p + 'rois'].any(axis=2).sum(axis=1)
        seen.add('proposal_more_columns_than_survivors' if (real < cfg['NMS_POST_MAXSIZE']).all() else 'proposal_full')
    return seen, shapes
