"""A numpy restatement of the contract of csrc/center_head.hip (include/pda_train.h, pda_center_*): target assignment, the two
losses with their gradients, and the decoding behind the top-k selection.  tests/test_center_head.py checks it against
tests/golden/center_head.npz (the reference's own output) on a machine without a GPU, so the contract the kernels are
written to is pinned there; the GPU tests then compare the kernels with the same fixture.

Every target operation is a float32 one in the order the header states; log, cos, sin, exp, atan2 and the Gaussian are
evaluated in float64 and rounded once."""
import numpy as np

F = np.float32


def head_layout(class_names, class_names_each_head):
    """label (1-based) -> (head, index inside the head)."""
    lay = {}
    for h, names in enumerate(class_names_each_head):
        for j, name in enumerate(names):
            lay[list(class_names).index(name) + 1] = (h, j)
    return lay


def gaussian_radius_f32(h, w, o):
    one_minus, one_plus = F(1.0 - o), F(1.0 + o)
    hw = F(h + w)
    c1 = F(F(F(w * h) * one_minus) / one_plus)
    r1 = F(F(hw + np.sqrt(F(F(hw * hw) - F(F(4) * c1)))) / F(2))
    b2 = F(F(2) * hw)
    c2 = F(F(one_minus * w) * h)
    r2 = F(F(b2 + np.sqrt(F(F(b2 * b2) - F(F(16) * c2)))) / F(2))
    b3 = F(F(-2.0 * o) * hw)
    c3 = F(F(F(o - 1.0) * w) * h)
    r3 = F(F(b3 + np.sqrt(F(F(b3 * b3) - F(F(4.0 * (4.0 * o)) * c3)))) / F(2))
    return min(r1, r2, r3)


def assign_targets(gt, class_names, class_names_each_head, hw, point_cloud_range, voxel_size, stride, max_objs, overlap, min_radius):
    """gt (B, M, cols) float32 -> per head (heatmaps, target_boxes, inds, masks)."""
    H, W = hw
    B, M, cols = gt.shape
    lay = head_layout(class_names, class_names_each_head)
    pcr0, pcr1, vs0, vs1, st = F(point_cloud_range[0]), F(point_cloud_range[1]), F(voxel_size[0]), F(voxel_size[1]), F(stride)
    out = []
    with np.errstate(all='ignore'):
        for h, names in enumerate(class_names_each_head):
            hm = np.zeros((B, len(names), H, W), F)
            tb = np.zeros((B, max_objs, cols), F)
            inds = np.zeros((B, max_objs), np.int64)
            masks = np.zeros((B, max_objs), np.int64)
            for b in range(B):
                rows = [r for r in gt[b] if lay.get(int(r[-1]), (-1, 0))[0] == h][:max_objs]
                for k, r in enumerate(rows):
                    x = F(F(F(r[0] - pcr0) / vs0) / st)
                    y = F(F(F(r[1] - pcr1) / vs1) / st)
                    x = min(max(x, F(0)), F(W - 0.5))
                    y = min(max(y, F(0)), F(H - 0.5))
                    cx, cy = int(x), int(y)
                    dx, dy = F(F(r[3] / vs0) / st), F(F(r[4] / vs1) / st)
                    if not (dx > 0 and dy > 0):
                        continue
                    rad = gaussian_radius_f32(dx, dy, overlap)
                    rad = max(int(rad), min_radius) if np.isfinite(rad) else min_radius
                    inds[b, k], masks[b, k] = cy * W + cx, 1
                    tb[b, k, 0], tb[b, k, 1], tb[b, k, 2] = F(x - F(cx)), F(y - F(cy)), r[2]
                    tb[b, k, 3:6] = np.log(r[3:6].astype(np.float64)).astype(F)
                    tb[b, k, 6], tb[b, k, 7] = F(np.cos(np.float64(r[6]))), F(np.sin(np.float64(r[6])))
                    tb[b, k, 8:] = r[7:-1]
                    left, right = min(cx, rad), min(W - cx, rad + 1)
                    top, bottom = min(cy, rad), min(H - cy, rad + 1)
                    if left + right <= 0 or top + bottom <= 0:
                        continue
                    sigma = (2 * rad + 1) / 6.0
                    jj, ii = np.mgrid[-top:bottom, -left:right].astype(np.float64)
                    g = np.exp(-(ii * ii + jj * jj) / (2.0 * sigma * sigma)).astype(F)
                    plane = hm[b, lay[int(r[-1])][1], cy - top:cy + bottom, cx - left:cx + right]
                    np.maximum(plane, g, out=plane)
            out.append((hm, tb, inds, masks))
    return out


def focal_loss(logits, heatmap):
    """(loss, d loss / d logits), sums in float64."""
    x = logits.astype(F)
    with np.errstate(all='ignore'):
        p = (F(1) / (F(1) + np.exp(-x))).astype(F)
    lo, hi = F(1e-4), F(1.0 - 1e-4)
    inside = (p >= lo) & (p <= hi)
    p = np.clip(p, lo, hi).astype(np.float64)
    t = heatmap.astype(np.float64)
    pos, neg = t == 1, t < 1
    q = 1.0 - p
    w = (1.0 - t) ** 4
    pos_sum = np.sum(np.where(pos, np.log(p) * q * q, 0.0))
    neg_sum = np.sum(np.where(neg, np.log(q) * p * p * w, 0.0))
    num = float(pos.sum())
    d = np.where(pos, q * q / p - 2.0 * q * np.log(p), np.where(neg, w * (2.0 * p * np.log(q) - p * p / q), 0.0))
    d = d * np.where(inside, p * q, 0.0)
    scale = -1.0 if num == 0 else -1.0 / num
    loss = -neg_sum if num == 0 else -(pos_sum + neg_sum) / num
    return loss, d * scale


def reg_loss(maps, masks, inds, targets, code_weights, loc_weight):
    """maps: list of (B, c, H, W) -> (loc_loss, [grad of every map])."""
    B, K, code = targets.shape
    cat = np.concatenate([m.reshape(B, m.shape[1], -1) for m in maps], axis=1).astype(np.float64)
    grad = np.zeros_like(cat)
    num = max(float(masks.sum()), 1.0)
    cols = np.zeros(code)
    for b in range(B):
        for k in range(K):
            if not masks[b, k]:
                continue
            for c in range(code):
                t = targets[b, k, c]
                if np.isnan(t):
                    continue
                d = cat[b, c, inds[b, k]] - np.float64(t)
                cols[c] += abs(d)
                grad[b, c, inds[b, k]] += np.sign(d) * code_weights[c] * loc_weight / num
    loss = float(np.sum(cols / num * np.asarray(code_weights, np.float64)) * loc_weight)
    out, at = [], 0
    for m in maps:
        out.append(grad[:, at:at + m.shape[1]].reshape(m.shape))
        at += m.shape[1]
    return loss, out


def decode(pred, K, class_map, point_cloud_range, voxel_size, stride, limit, score_thresh):
    """pred: a head's maps -> (flat top-K indices (B, K), boxes (B, K, 7 | 9), scores (B, K) with -inf for masked rows,
    labels (B, K))."""
    hm = pred['hm']
    B, C, H, W = hm.shape
    flat = hm.reshape(B, -1)
    ind = np.argsort(-flat, axis=1, kind='stable')[:, :K]
    top = np.take_along_axis(flat, ind, axis=1)
    cls, cell = ind // (H * W), ind % (H * W)
    cell_y, cell_x = (cell // W).astype(F), (cell % W).astype(F)

    def at(m, c):
        return np.take_along_axis(m[:, c].reshape(B, -1), cell, axis=1)
    st, vs0, vs1, p0, p1 = F(stride), F(voxel_size[0]), F(voxel_size[1]), F(point_cloud_range[0]), F(point_cloud_range[1])
    xs = ((cell_x + at(pred['center'], 0)) * st * vs0 + p0).astype(F)
    ys = ((cell_y + at(pred['center'], 1)) * st * vs1 + p1).astype(F)
    zs = at(pred['center_z'], 0)
    parts = [xs, ys, zs] + [np.exp(at(pred['dim'], c).astype(np.float64)).astype(F) for c in range(3)]
    parts.append(np.arctan2(at(pred['rot'], 1).astype(np.float64), at(pred['rot'], 0).astype(np.float64)).astype(F))
    if 'vel' in pred:
        parts += [at(pred['vel'], 0), at(pred['vel'], 1)]
    boxes = np.stack(parts, axis=-1)
    with np.errstate(all='ignore'):
        scores = (F(1) / (F(1) + np.exp(-top.astype(F)))).astype(F)
    lim = np.asarray(limit, F)
    ok = (boxes[..., :3] >= lim[:3]).all(-1) & (boxes[..., :3] <= lim[3:]).all(-1)
    if score_thresh is not None:
        ok &= scores > F(score_thresh)
    return ind, boxes, np.where(ok, scores, F(-np.inf)).astype(F), np.asarray(class_map, np.int64)[cls]
