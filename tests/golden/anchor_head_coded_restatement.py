"""A numpy restatement of the contract of the `_coded` anchor-head entries (include/pda_train.h): ResidualCoder with
encode_angle_by_sincos and custom columns, WeightedL1Loss next to the smooth L1, and the decode.  It builds on
anchor_head_restatement.py (IoU, the plain encode, the direction bins).  extra = gt columns - 8, sincos 0 or 1, a code row holds
6 + (2 if sincos else 1) + extra columns.  Float32 where the header says so -- every cosine, sine and atan2 evaluated in float64
and rounded once --, the losses and their gradients in float64.  tests/test_anchor_head_coded.py checks it against
tests/golden/anchor_head_coded.npz (the reference's own output) without a GPU and the kernels against both."""
import numpy as np

import anchor_head_restatement as rs

F = np.float32


def code_width(gt_cols, sincos):
    return 6 + (2 if sincos else 1) + (gt_cols - 8)


def encode(gt, anchor, sincos):
    """ResidualCoder.encode_torch for one gt row (7 + extra + 1 columns) against one 7-column anchor (its custom columns 0)."""
    extra = len(gt) - 8
    plain = rs.encode(gt, anchor)
    if sincos:
        angle = [F(F(np.cos(np.float64(gt[6]))) - F(np.cos(np.float64(anchor[6])))),
                 F(F(np.sin(np.float64(gt[6]))) - F(np.sin(np.float64(anchor[6]))))]
    else:
        angle = [plain[6]]
    return np.concatenate([plain[:6], np.array(angle, F), np.asarray(gt[7:7 + extra], F)])


def row_classes(class_counts, n_rows, class_major):
    """The anchor class of every row of the table: class c owns class_counts[c] contiguous rows (class-major) or that many
    slots of every location (location-major)."""
    if class_major:
        return np.repeat(np.arange(len(class_counts)), class_counts)
    slot_class = np.repeat(np.arange(len(class_counts)), class_counts)
    return slot_class[np.arange(n_rows) % len(slot_class)]


def assign_targets(gt, table, class_label, matched, unmatched, class_counts, sincos, class_major=True):
    """gt (B, M, 8 + extra), table (N, 7).  Returns labels (B, N) int32, targets (B, N, code), weights (B, N), num_pos (B) int32:
    the rule of anchor_head_restatement.assign_targets per (scene, class, anchor), the IoUs on columns 0..6."""
    gt, table = np.asarray(gt, F), np.asarray(table, F)
    B, N = gt.shape[0], table.shape[0]
    code = code_width(gt.shape[2], sincos)
    cls_of = row_classes(class_counts, N, class_major)
    assert len(cls_of) == N
    labels = np.zeros((B, N), np.int32)
    targets = np.zeros((B, N, code), F)
    weights = np.zeros((B, N), F)
    for s in range(B):
        last = gt[s, :, -1]
        glab = np.where(last >= 1, last, 0).astype(np.int64)
        for c in range(len(class_label)):
            rows = np.nonzero(cls_of == c)[0]
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
                targets[s, rows[i]] = encode(gt[s, cols[row_arg[i]]], table[rows[i]], sincos)
                weights[s, rows[i]] = 1
    return labels, targets, weights, (labels > 0).sum(axis=1).astype(np.int32)


def losses(cls_preds, box_preds, dir_preds, head_cols, head_col_base, labels, targets, table, num_class, code_weights, cls_weight,
           loc_weight, dir_weight=0.0, dir_offset=0.0, pos_cls_weight=1.0, neg_cls_weight=1.0, sincos=0, l1=False, sin_diff=None):
    """([rpn_loss_cls, rpn_loss_loc, rpn_loss_dir, rpn_loss], grads) in float64 from lists of per-head predictions (B, N_h, C_h),
    (B, N_h, code), (B, N_h, bins) | dir_preds None; grads = (per-head d rpn_loss / d cls, d box, d dir | None).  l1:
    WeightedL1Loss (gradient sign(diff) * code_weight, 0 at diff == 0), else smooth L1 with beta 1/9.  A NaN target gives 0 in
    the loss and the gradient.  sin_diff (None: behind a direction classifier, as the multihead does): the sine difference on
    column 6; never with sincos."""
    B, N = labels.shape
    code = targets.shape[-1]
    cw = np.asarray(code_weights, np.float64)
    assert len(cw) == code and not (sincos and dir_preds is not None)
    sin_diff = (dir_preds is not None) if sin_diff is None else sin_diff
    norm = np.maximum((labels > 0).sum(axis=1, keepdims=True), 1).astype(np.float64)
    start = 0
    cls = loc = dl = 0.0
    g_cls, g_box, g_dir = [], [], []
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
        dpt = np.where(t > 0, -p * (1 - p), p * (1 - p))
        g_cls.append(alpha * (2 * pt * dpt * bce + pt ** 2 * (p - t)) * w * cls_weight / B)
        pos = (lab > 0) / norm
        bp = np.asarray(box_preds[h], np.float64).reshape(B, n, code).copy()
        tg = np.asarray(targets[:, start:start + n], np.float64).copy()
        chain = np.ones_like(bp)
        if sin_diff and not sincos:
            a, b = bp[..., 6].copy(), tg[..., 6].copy()
            bp[..., 6], tg[..., 6] = np.sin(a) * np.cos(b), np.cos(a) * np.sin(b)
            chain[..., 6] = np.cos(a) * np.cos(b) + np.sin(a) * np.sin(b)
        nan = np.isnan(tg)
        diff = np.where(nan, 0, bp - np.where(nan, 0, tg)) * cw
        ad, beta = np.abs(diff), 1.0 / 9.0
        if l1:
            term, slope = ad, np.sign(diff)
        else:
            term, slope = np.where(ad < beta, 0.5 * ad ** 2 / beta, ad - 0.5 * beta), np.where(ad < beta, diff / beta, np.sign(diff))
        loc += (term * pos[..., None]).sum() / B * loc_weight
        g_box.append(np.where(nan, 0, slope * cw * chain) * pos[..., None] * loc_weight / B)
        if dir_preds is not None:
            d = np.asarray(dir_preds[h], np.float64).reshape(B, n, -1)
            bins = rs.direction_bins(targets[:, start:start + n], table[start:start + n], dir_offset, d.shape[-1])
            mx = d.max(axis=-1, keepdims=True)
            lse = mx + np.log(np.exp(d - mx).sum(axis=-1, keepdims=True))
            dl += ((lse[..., 0] - np.take_along_axis(d, bins[..., None], axis=-1)[..., 0]) * pos).sum() / B * dir_weight
            one_hot = (bins[..., None] == np.arange(d.shape[-1])).astype(np.float64)
            g_dir.append((np.exp(d - lse) - one_hot) * pos[..., None] * dir_weight / B)
        start += n
    assert start == N
    return np.array([cls, loc, dl, cls + loc + dl]), (g_cls, g_box, g_dir if dir_preds is not None else None)


def decode(box_preds, dir_preds, table, dir_offset=0.0, dir_limit_offset=0.0, sincos=0):
    """generate_predicted_boxes: (B, N, code) -> (B, N, code - sincos) float32."""
    table = np.asarray(table, F)
    B, N = np.asarray(box_preds).shape[0], table.shape[0]
    t = np.asarray(box_preds, F).reshape(B, N, -1)
    angle = 2 if sincos else 1
    extra = t.shape[2] - 6 - angle
    plain = np.concatenate([t[..., :6], t[..., 6:7] if not sincos else np.zeros_like(t[..., :1])], axis=-1)
    out = np.zeros((B, N, 7 + extra), F)
    out[..., :7] = rs.decode(plain, None if sincos else dir_preds, table, dir_offset, dir_limit_offset)
    if sincos:
        assert dir_preds is None
        ra = table[None, :, 6].astype(np.float64)
        sn = t[..., 7] + np.sin(ra).astype(F)
        cs = t[..., 6] + np.cos(ra).astype(F)
        out[..., 6] = np.arctan2(sn.astype(np.float64), cs.astype(np.float64)).astype(F)
    out[..., 7:] = t[..., 6 + angle:] + F(0)
    return out
