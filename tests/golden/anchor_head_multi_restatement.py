"""A numpy restatement of the contract of pda_anchor_multi_assign_targets and pda_anchor_multi_loss (include/pda_train.h), next
to anchor_head_restatement.py, whose IoU, box encoding and direction bins it uses: the class-major anchor table of
USE_MULTIHEAD, target assignment by row segment, and the losses of heads whose logits have different column counts.
tests/test_anchor_head_multi.py checks it against tests/golden/anchor_head_multi.npz (the reference's own output) without a
GPU; the GPU tests then compare the kernels with the same fixture.  Float32 where the header says so, the losses in float64."""
import numpy as np

import anchor_head_restatement as rs

F = np.float32


def class_major_table(anchors):
    """Per class (1, ny, nx, n_sizes, n_rot, 7) -> the (N, 7) table and the rows of each class: permute(3, 4, 0, 1, 2, 5)."""
    flat = [np.ascontiguousarray(np.transpose(a, (3, 4, 0, 1, 2, 5))).reshape(-1, 7) for a in anchors]
    return np.concatenate(flat, axis=0), [len(f) for f in flat]


def assign_targets(gt, table, class_label, matched, unmatched, class_rows):
    """rs.assign_targets with class c owning the class_rows[c] contiguous rows behind those of the classes before it."""
    gt, table = np.asarray(gt, F), np.asarray(table, F)
    B, N = gt.shape[0], table.shape[0]
    first = np.concatenate([[0], np.cumsum(class_rows)])
    assert first[-1] == N
    labels = np.zeros((B, N), np.int32)
    targets = np.zeros((B, N, 7), F)
    weights = np.zeros((B, N), F)
    for s in range(B):
        glab = np.where((gt[s, :, 7] >= 1), gt[s, :, 7], 0).astype(np.int64)
        for c in range(len(class_label)):
            rows = np.arange(first[c], first[c + 1])
            cols = np.nonzero(glab == class_label[c])[0]           # a label-0 row takes part in no class
            if len(cols) == 0:
                continue
            iou = rs.nearest_bev_iou(table[rows], gt[s, cols, :7])
            row_arg = iou.argmax(axis=1)                            # the lowest index on a tie
            row_max = iou[np.arange(len(rows)), row_arg]
            col_max = iou.max(axis=0)
            col_max = np.where(col_max == 0, F(-1), col_max)
            forced = (iou == col_max[None, :]).any(axis=1)
            lab = np.full(len(rows), -1, np.int32)
            lab[row_max >= F(matched[c])] = class_label[c]
            lab[row_max < F(unmatched[c])] = 0
            lab[forced] = class_label[c]
            labels[s, rows] = lab
            for i in np.nonzero(lab > 0)[0]:
                targets[s, rows[i]] = rs.encode(gt[s, cols[row_arg[i]]], table[rows[i]])
                weights[s, rows[i]] = 1
    return labels, targets, weights, (labels > 0).sum(axis=1).astype(np.int32)


def losses(cls_preds, box_preds, dir_preds, head_cols, head_col_base, labels, targets, table, num_class, code_weights, cls_weight,
           loc_weight, dir_weight=0.0, dir_offset=0.0, pos_cls_weight=1.0, neg_cls_weight=1.0):
    """[rpn_loss_cls, rpn_loss_loc, rpn_loss_dir, rpn_loss] in float64 from lists of per-head predictions (B, N_h, C_h),
    (B, N_h, 7), (B, N_h, bins) | dir_preds None.  The normaliser is the scene's positives over ALL heads; the sin difference is
    taken only behind a direction classifier."""
    B, N = labels.shape
    norm = np.maximum((labels > 0).sum(axis=1, keepdims=True), 1).astype(np.float64)
    start = 0
    cls = loc = dl = 0.0
    for h, x in enumerate(cls_preds):
        x = np.asarray(x, np.float64)
        n = x.shape[1]
        lab = labels[:, start:start + n]
        hot = np.where(lab > 0, 0 if num_class == 1 else lab - 1 - head_col_base[h], -1)
        t = (hot[..., None] == np.arange(head_cols[h])[None, None, :]).astype(np.float64)
        p = 1 / (1 + np.exp(-x))
        alpha = t * 0.25 + (1 - t) * 0.75
        pt = t * (1 - p) + (1 - t) * p
        bce = np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))
        w = (((lab > 0) * pos_cls_weight + (lab == 0) * neg_cls_weight) / norm)[..., None]
        cls += (alpha * pt ** 2 * bce * w).sum() / B * cls_weight
        pos = (lab > 0) / norm
        bp = np.asarray(box_preds[h], np.float64).reshape(B, n, 7).copy()
        tg = np.asarray(targets[:, start:start + n], np.float64).copy()
        if dir_preds is not None:
            a, b = bp[..., 6].copy(), tg[..., 6].copy()
            bp[..., 6], tg[..., 6] = np.sin(a) * np.cos(b), np.cos(a) * np.sin(b)
        diff = np.where(np.isnan(tg), 0, bp - tg) * np.asarray(code_weights, np.float64)
        ad, beta = np.abs(diff), 1.0 / 9.0
        loc += (np.where(ad < beta, 0.5 * ad ** 2 / beta, ad - 0.5 * beta) * pos[..., None]).sum() / B * loc_weight
        if dir_preds is not None:
            d = np.asarray(dir_preds[h], np.float64).reshape(B, n, -1)
            bins = rs.direction_bins(targets[:, start:start + n], table[start:start + n], dir_offset, d.shape[-1])
            mx = d.max(axis=-1, keepdims=True)
            lse = (mx + np.log(np.exp(d - mx).sum(axis=-1, keepdims=True)))[..., 0]
            dl += ((lse - np.take_along_axis(d, bins[..., None], axis=-1)[..., 0]) * pos).sum() / B * dir_weight
        start += n
    assert start == N
    return np.array([cls, loc, dl, cls + loc + dl])
