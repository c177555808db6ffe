"""random_local_pyramid_aug as the device runs it (include/pda_train.h pda_pyramid_aug, csrc/augment_steps.hip), restated in
float32 numpy: every line a separately rounded operation, the departures from the reference included (a scene never grows:
a self pair and a pair whose partner pyramid an earlier pair holds do nothing, a point in pyramids of several pairs is moved
by the first, points leave in scene order, C > 4 keeps the middle columns).  tests/test_pyramid_aug.py holds the kernel to
this bit for bit, and this to the reference's recorded scenes."""
import numpy as np

f32 = np.float32
ORDERS = np.array([[0, 1, 5, 4], [4, 5, 6, 7], [7, 6, 2, 3], [3, 2, 1, 0], [1, 2, 6, 5], [0, 4, 7, 3]])
TEMPLATE = np.array([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]], f32) / f32(2)
_M32 = 0xffffffff


def _cs(a):
    return f32(np.cos(np.float64(a))), f32(np.sin(np.float64(a)))


def faces(points, box):
    """The pyramid of `box` every point lies in (0 +x, 1 +z, 2 -x, 3 -z, 4 -y, 5 +y), -1 outside the box."""
    P = np.asarray(points, f32)
    b = np.asarray(box, f32)
    cosa, sina = _cs(-b[6])
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (P[:, 2] - b[2]) / (b[5] / f32(2))
        sx, sy = P[:, 0] - b[0], P[:, 1] - b[1]
        u = (sx * cosa + sy * (-sina)) / (b[3] / f32(2))
        v = (sx * sina + sy * cosa) / (b[4] / f32(2))
    au, av, aw = np.abs(u), np.abs(v), np.abs(w)
    inside = (au <= 1) & (av <= 1) & (aw <= 1)
    fx = np.where(u >= 0, 0, 2)
    fz = np.where(w >= 0, 1, 3)
    fy = np.where(v >= 0, 5, 4)
    f = np.where((au >= av) & (au >= aw), fx, np.where(aw >= av, fz, fy))
    return np.where(inside, f, -1)


def _mix32(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & _M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & _M32
    x ^= x >> 16
    return x


def keyed_bijection(key, m, x):
    """csrc/stage_rng.h keyed_bijection."""
    key, m, x = int(key), int(m), int(x)
    h = 1
    while (1 << (2 * h)) < m:
        h += 1
    mask = (1 << h) - 1
    k0, k1 = key & _M32, (key >> 32) & _M32
    while True:
        l, r = x >> h, x & mask
        for rnd in range(6):
            f = _mix32(r ^ _mix32(((k1 if rnd & 1 else k0) + 0x9e3779b9 * (rnd + 1)) & _M32)) & mask
            l, r = r, l ^ f
        x = (l << h) | r
        if x < m:
            return x


def frame(box, face):
    """c0, v0, v1, surface centre, v2, |v0|^2, |v1|^2, |v2|^2 of one pyramid (boxes_to_corners_3d in float32)."""
    b = np.asarray(box, f32)
    c, s = _cs(b[6])
    cr = []
    for k in ORDERS[face]:
        tx, ty, tz = b[3] * TEMPLATE[k, 0], b[4] * TEMPLATE[k, 1], b[5] * TEMPLATE[k, 2]
        cr.append(np.array([(tx * c + ty * (-s)) + b[0], (tx * s + ty * c) + b[1], tz + b[2]], f32))
    sc = (((cr[0] + cr[1]) + cr[2]) + cr[3]) / f32(4)
    v0, v1, v2 = cr[1] - cr[0], cr[3] - cr[0], b[:3] - sc
    n = [(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] for v in (v0, v1, v2)]
    return cr[0], v0, v1, sc, v2, n[0], n[1], n[2]


def _dot(d, v):
    return (d[:, 0] * v[0] + d[:, 1] * v[1]) + d[:, 2] * v[2]


def swap_points(P, fr, to, mm_from, mm_to):
    """Rows P (n, C) of pyramid `fr` by their ratios in pyramid `to`; the last column to the range of `to`."""
    c0, v0, v1, sc, v2, n0, n1, n2 = fr
    al = _dot(P[:, :3] - c0, v0) / n0
    be = _dot(P[:, :3] - c0, v1) / n1
    ga = _dot(P[:, :3] - sc, v2) / n2
    t0, w0, w1, _, w2 = to[:5]
    out = P.copy()
    for a in range(3):
        out[:, a] = ((al * w0[a] + be * w1[a]) + t0[a]) + ga * w2[a]
    ratio = (P[:, -1] - mm_from[0]) / np.clip(mm_from[1] - mm_from[0], f32(1e-6), f32(1))
    out[:, -1] = ratio * (mm_to[1] - mm_to[0]) + mm_to[0]
    return out


def pyramid_aug(points, boxes8, cfg, draws):
    """One scene.  points (n, C) float32; boxes8 (m, 8) with the class column, class 0 included; cfg: drop_prob,
    sparsify_prob, sparsify_max, swap_prob, swap_max; draws: the scene's rows of the plan (pyramid_* without the prefix:
    drop_face, drop_u, sparsify_face, sparsify_u, sparsify_key, sparsify_keep, swap_u, swap_face_u, swap_partner_u,
    swap_face, swap_partner; the optional ones may be missing).
    -> points out (scene order), boxes out (limit_period, class 0 dropped), trace: dict(bad=, dropped=, thinned=,
    selected_not_thinned=, pairs=[(box, face, partner, active)], no_face=, moved= (n_out) bool, src= (n_out) input rows)."""
    P = np.array(points, f32)
    bx = np.array(boxes8, f32).reshape(-1, 8)
    n, m = len(P), len(bx)
    tr = dict(bad=False, dropped=0, thinned=0, selected_not_thinned=0, pairs=[], no_face=0)
    get = lambda k: np.asarray(draws[k]).reshape(-1) if draws.get(k) is not None else None
    F = [faces(P, b) for b in bx]
    alive = np.ones(n, bool)
    bad = False
    # 1. dropout
    dface, du = get("drop_face"), get("drop_u")
    if len(du) < m or ((dface[:m] < 0) | (dface[:m] > 5)).any():
        bad = True
    left1 = []
    if not bad:
        for i in range(m):
            if du[i] <= cfg["drop_prob"]:
                alive &= F[i] != dface[i]
                tr["dropped"] += 1
            else:
                left1.append(i)
    # 2. sparsify
    sface, su, skey, skeep = get("sparsify_face"), get("sparsify_u"), get("sparsify_key"), draws.get("sparsify_keep")
    if not bad and (len(su) < len(left1) or ((sface[:len(left1)] < 0) | (sface[:len(left1)] > 5)).any()):
        bad = True
    left2 = []
    in_thin, kept = np.zeros(n, bool), np.zeros(n, bool)
    if not bad:
        for j, i in enumerate(left1):
            if not su[j] <= cfg["sparsify_prob"]:
                left2.append(i)
                continue
            rows = np.nonzero(alive & (F[i] == sface[j]))[0]
            cnt = len(rows)
            if cnt <= cfg["sparsify_max"]:
                tr["selected_not_thinned"] += 1
                continue
            tr["thinned"] += 1
            lst = np.asarray(skeep[j], np.int64).reshape(-1) if skeep is not None and j < len(skeep) else np.zeros(0, np.int64)
            if len(lst):
                if len(lst) != cfg["sparsify_max"] or len(set(lst.tolist())) != len(lst) or (lst < 0).any() or (lst >= cnt).any():
                    bad = True
                    break
                keep_rank = np.isin(np.arange(cnt), lst)
            else:
                key = skey[j] if skey is not None and j < len(skey) else 0
                keep_rank = np.array([keyed_bijection(key, cnt, r) < cfg["sparsify_max"] for r in range(cnt)], bool)
            in_thin[rows] = True
            kept[rows[keep_rank]] = True
    alive2 = alive & (~in_thin | kept)
    # 3. swap
    swu = get("swap_u")
    if not bad and len(swu) < len(left2):
        bad = True
    owner, pair = {}, {}
    if not bad:
        L = len(left2)
        ov_f, ov_p = get("swap_face"), get("swap_partner")
        fu, pu = get("swap_face_u"), get("swap_partner_u")
        at = lambda a, k, d: a[k] if a is not None and k < len(a) else d
        I = P[:, -1]
        cnt = np.zeros((m, 6), np.int64)
        mm = {}
        for i in left2:
            for f in range(6):
                sel = alive2 & (F[i] == f)
                cnt[i, f] = sel.sum()
                if cnt[i, f]:
                    mm[(i, f)] = (I[sel].min(), I[sel].max())
        face = {}
        for k, i in enumerate(left2):
            if not swu[k] <= cfg["swap_prob"]:
                continue
            valid = [f for f in range(6) if cnt[i, f] > cfg["swap_max"]]
            o = int(at(ov_f, k, -1))
            if o >= 0:
                if o in valid:
                    face[i] = o
                else:
                    bad = True
            elif valid:
                face[i] = valid[min(int(np.float64(at(fu, k, 0.0)) * len(valid)), len(valid) - 1)]
            else:
                tr["no_face"] += 1
        partner = {}
        for k, i in enumerate(left2):
            if i not in face:
                continue
            j = face[i]
            cand = [q for q in left2 if cnt[q, j] > cfg["swap_max"] and face.get(q, -1) != j]
            o = int(at(ov_p, k, -1))
            if o >= 0:
                q = left2[o] if o < L else -1
                if q >= 0 and (q in cand if cand else q == i):
                    partner[i] = q
                else:
                    bad = True
            elif not cand:
                partner[i] = i
            else:
                partner[i] = cand[min(int(np.float64(at(pu, k, 0.0)) * len(cand)), len(cand) - 1)]
        taken = set()
        for i in left2:
            if i not in partner:
                continue
            j, q = face[i], partner[i]
            active = q != i and (q, j) not in taken
            taken.add((q, j))
            tr["pairs"].append((i, j, q, bool(active)))
            if active:
                owner[(i, j)] = owner[(q, j)] = i
                pair[i] = (j, q)
    tr["bad"] = bad
    two_pi = f32(6.28318530717958647692)
    fin = bx[bx[:, 7] != 0].copy()
    fin[:, 6] = fin[:, 6] - np.floor(fin[:, 6] / two_pi + f32(0.5)) * two_pi
    if bad:
        tr.update(moved=np.zeros(0, bool), src=np.zeros(0, np.int64))
        return P[:0], fin[:0], tr
    out = P.copy()
    moved = np.zeros(n, bool)
    if pair:
        own = np.full(n, m, np.int64)
        pyr = np.full((n, 2), -1, np.int64)
        for i in left2:
            for f in range(6):
                o = owner.get((i, f))
                if o is None:
                    continue
                hit = alive2 & (F[i] == f) & (o < own)
                own[hit] = o
                pyr[hit] = (i, f)
        for i, (j, q) in pair.items():
            fa, fp = frame(bx[i], j), frame(bx[q], j)
            ra = (own == i) & (pyr[:, 0] == i) & (pyr[:, 1] == j)
            rp = (own == i) & ~ra
            out[ra] = swap_points(P[ra], fa, fp, mm[(i, j)], mm[(q, j)])
            out[rp] = swap_points(P[rp], fp, fa, mm[(q, j)], mm[(i, j)])
            moved |= ra | rp
    tr.update(moved=moved[alive2], src=np.nonzero(alive2)[0])
    return out[alive2], fin, tr
