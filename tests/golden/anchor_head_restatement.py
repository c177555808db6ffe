"""A numpy restatement of the contract of csrc/anchor_head.hip (include/pda_train.h, pda_anchor_* and pda_pillar_features):
the nearest-BEV IoU, target assignment, the three losses, the box decoding and the PFN input rows.
tests/test_anchor_head.py and tests/test_pillar_vfe.py check it against tests/golden/anchor_head.npz (the reference's own
output) on a machine without a GPU, so the contract the kernels are written to is pinned there; the GPU tests then compare
the kernels with the same fixture.

Every IoU and target operation is a float32 one in the order the header states (numpy rounds each float32 operation
separately); log and exp are evaluated in float64 and rounded once; the losses are evaluated in float64."""
import numpy as np

F = np.float32
PI = F(np.pi)


def aligned_bev(boxes):
    """(n, >= 7) float32 -> (n, 4) [x1, y1, x2, y2]: boxes3d_lidar_to_aligned_bev_boxes."""
    boxes = np.asarray(boxes, F)
    ry = boxes[:, 6]
    r = np.abs(ry - np.floor(ry / PI + F(0.5)) * PI)
    keep = r < F(np.pi / 4)
    cx = np.where(keep, boxes[:, 3], boxes[:, 4])
    cy = np.where(keep, boxes[:, 4], boxes[:, 3])
    hx, hy = cx / F(2), cy / F(2)
    return np.stack([boxes[:, 0] - hx, boxes[:, 1] - hy, boxes[:, 0] + hx, boxes[:, 1] + hy], axis=1).astype(F)


def nearest_bev_iou(anchors, gts):
    """(n, 7), (m, 7) -> (n, m) float32: boxes3d_nearest_bev_iou."""
    a, b = aligned_bev(anchors), aligned_bev(gts)
    x_min = np.maximum(a[:, None, 0], b[None, :, 0])
    x_max = np.minimum(a[:, None, 2], b[None, :, 2])
    y_min = np.maximum(a[:, None, 1], b[None, :, 1])
    y_max = np.minimum(a[:, None, 3], b[None, :, 3])
    x_len = np.maximum(x_max - x_min, F(0))
    y_len = np.maximum(y_max - y_min, F(0))
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    inter = x_len * y_len
    return (inter / np.maximum(area_a[:, None] + area_b[None, :] - inter, F(1e-6))).astype(F)


def encode(gt, anchor):
    """ResidualCoder.encode_torch for one pair of rows."""
    dxa, dya, dza = (max(F(anchor[i]), F(1e-5)) for i in (3, 4, 5))
    dxg, dyg, dzg = (max(F(gt[i]), F(1e-5)) for i in (3, 4, 5))
    diagonal = np.sqrt(F(F(dxa * dxa) + F(dya * dya)))
    t = np.zeros(7, F)
    t[0] = F(gt[0] - anchor[0]) / diagonal
    t[1] = F(gt[1] - anchor[1]) / diagonal
    t[2] = F(gt[2] - anchor[2]) / dza
    t[3] = F(np.log(np.float64(F(dxg / dxa))))
    t[4] = F(np.log(np.float64(F(dyg / dya))))
    t[5] = F(np.log(np.float64(F(dzg / dza))))
    t[6] = F(gt[6] - anchor[6])
    return t


def assign_targets(gt, table, class_label, matched, unmatched, class_count):
    """gt (B, M, 8), table (N, 7) the anchors in target order; per anchor class its label, thresholds and slot count.
    Returns labels (B, N) int32, targets (B, N, 7), weights (B, N), num_pos (B) int32."""
    gt, table = np.asarray(gt, F), np.asarray(table, F)
    B, M, _ = gt.shape
    N = table.shape[0]
    slots = int(sum(class_count))
    slot_class = np.concatenate([np.full(k, c) for c, k in enumerate(class_count)])
    cls_of = slot_class[np.arange(N) % slots]
    labels = np.zeros((B, N), np.int32)
    targets = np.zeros((B, N, 7), F)
    weights = np.zeros((B, N), F)
    for s in range(B):
        glab = np.where((gt[s, :, 7] >= 1), gt[s, :, 7], 0).astype(np.int64)
        for c in range(len(class_label)):
            rows = np.nonzero(cls_of == c)[0]
            cols = np.nonzero(glab == class_label[c])[0]           # a label-0 row takes part in no class
            if len(cols) == 0 or len(rows) == 0:
                continue
            iou = nearest_bev_iou(table[rows], gt[s, cols, :7])
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
                targets[s, rows[i]] = encode(gt[s, cols[row_arg[i]]], table[rows[i]])
                weights[s, rows[i]] = 1
    return labels, targets, weights, (labels > 0).sum(axis=1).astype(np.int32)


def direction_bins(targets, table, dir_offset, bins):
    """get_direction_target without the one-hot: (B, N) int64, float32 arithmetic."""
    rot_gt = np.asarray(targets, F)[..., 6] + np.asarray(table, F)[None, :, 6]
    val = rot_gt - F(dir_offset)
    two_pi = F(2 * np.pi)
    offset_rot = val - np.floor(val / two_pi + F(0)) * two_pi
    return np.clip(np.floor(offset_rot / F(2 * np.pi / bins)).astype(np.int64), 0, bins - 1)


def losses(cls_preds, box_preds, dir_preds, labels, targets, table, num_class, code_weights, cls_weight, loc_weight,
           dir_weight=0.0, dir_offset=0.0):
    """[rpn_loss_cls, rpn_loss_loc, rpn_loss_dir, rpn_loss] in float64."""
    B, N = labels.shape
    x = np.asarray(cls_preds, np.float64).reshape(B, N, num_class)
    norm = np.maximum((labels > 0).sum(axis=1, keepdims=True), 1).astype(np.float64)
    hot_label = np.where(labels > 0, 1 if num_class == 1 else labels, 0)
    t = (hot_label[..., None] == np.arange(1, num_class + 1)[None, None, :]).astype(np.float64)
    p = 1 / (1 + np.exp(-x))
    alpha = t * 0.25 + (1 - t) * 0.75
    pt = t * (1 - p) + (1 - t) * p
    bce = np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))
    w = ((labels >= 0) / norm)[..., None]
    cls = (alpha * pt ** 2 * bce * w).sum() / B * cls_weight
    pos = ((labels > 0) / norm)
    bp, tg = np.asarray(box_preds, np.float64).reshape(B, N, 7).copy(), np.asarray(targets, np.float64).copy()
    a, b = bp[..., 6].copy(), tg[..., 6].copy()
    bp[..., 6], tg[..., 6] = np.sin(a) * np.cos(b), np.cos(a) * np.sin(b)
    diff = np.where(np.isnan(tg), 0, bp - tg) * np.asarray(code_weights, np.float64)
    ad, beta = np.abs(diff), 1.0 / 9.0
    loc = (np.where(ad < beta, 0.5 * ad ** 2 / beta, ad - 0.5 * beta) * pos[..., None]).sum() / B * loc_weight
    dl = 0.0
    if dir_preds is not None:
        d = np.asarray(dir_preds, np.float64).reshape(B, N, -1)
        bins = direction_bins(targets, table, dir_offset, d.shape[-1])
        mx = d.max(axis=-1, keepdims=True)
        lse = (mx + np.log(np.exp(d - mx).sum(axis=-1, keepdims=True)))[..., 0]
        dl = ((lse - np.take_along_axis(d, bins[..., None], axis=-1)[..., 0]) * pos).sum() / B * dir_weight
    return np.array([cls, loc, dl, cls + loc + dl])


def decode(box_preds, dir_preds, table, dir_offset=0.0, dir_limit_offset=0.0):
    """generate_predicted_boxes: (B, N, 7) float32."""
    table = np.asarray(table, F)
    B, N = np.asarray(box_preds).shape[0], table.shape[0]
    t = np.asarray(box_preds, F).reshape(B, N, 7)
    a = table[None]
    diagonal = np.sqrt(a[..., 3] * a[..., 3] + a[..., 4] * a[..., 4])
    out = np.zeros((B, N, 7), F)
    out[..., 0] = t[..., 0] * diagonal + a[..., 0]
    out[..., 1] = t[..., 1] * diagonal + a[..., 1]
    out[..., 2] = t[..., 2] * a[..., 5] + a[..., 2]
    for c in (3, 4, 5):
        out[..., c] = np.exp(t[..., c].astype(np.float64)).astype(F) * a[..., c]
    rg = t[..., 6] + a[..., 6]
    if dir_preds is not None:
        d = np.asarray(dir_preds, F).reshape(B, N, -1)
        period = F(2 * np.pi / d.shape[-1])
        best = d.argmax(axis=-1)
        val = rg - F(dir_offset)
        dir_rot = val - np.floor(val / period + F(dir_limit_offset)) * period
        rg = (dir_rot + F(dir_offset)) + period * best.astype(F)
    out[..., 6] = rg
    return out


def pillar_features(voxels, num_points, coords, voxel_size, point_cloud_range, use_absolute_xyz, with_distance):
    """(V, P, C) -> (V, P, C'): the sum behind the mean runs in row order."""
    vox = np.asarray(voxels, F)
    V, P, C = vox.shape
    total = np.zeros((V, 3), F)
    for p in range(P):
        total = total + vox[:, p, :3]
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = total / np.asarray(num_points).astype(F)[:, None]
    vs = [float(v) for v in voxel_size]
    off = [F(vs[i] / 2 + float(point_cloud_range[i])) for i in range(3)]
    centre = np.stack([np.asarray(coords)[:, 3 - i].astype(F) * F(vs[i]) + off[i] for i in range(3)], axis=1)
    parts = [vox if use_absolute_xyz else vox[..., 3:], vox[..., :3] - mean[:, None, :], vox[..., :3] - centre[:, None, :]]
    if with_distance:
        x, y, z = vox[..., 0], vox[..., 1], vox[..., 2]
        parts.append(np.sqrt((x * x + y * y) + z * z)[..., None])
    out = np.concatenate(parts, axis=-1).astype(F)
    out[np.arange(P)[None, :] >= np.asarray(num_points)[:, None]] = 0
    return out
