"""Seeded inputs of tests/test_roi_pool.py and make_roi_pool_golden.py: the smallest scenes that still reach every branch
of the RoI pooling kernels (csrc/roi_pool.hip).

`exact`: coordinates, box centres and sizes on the 1/8 lattice, heading 0: the local coordinates are exact in float32, so
no decision depends on the contraction mode.  Points lie exactly on box faces and on voxel boundaries.
`generic`: random headings, scenes within +-40 m.  The roiaware generator drops every candidate point that, for any box
and evaluated in float64, lies within DROP = 2e-4 m of a box face, of the box-test limit (face + 1e-5) or of a voxel
boundary of one of GRIDS.  Coordinates below 64 m have a float32 ulp of 3.8e-6 m and the local coordinates plus the index
expression accumulate fewer than five roundings, so 2e-4 m is more than 10x the worst case: no decision depends on the FMA
mode.  The generator asserts that it drops at most 5 % of the in-box (point, box) pairs (share: see roiaware_inputs.drop).
The roipoint scenes are built in the boxes' local frames with every point at least 0.04 m from every face of the plain
and the enlarged boxes, which the generator asserts."""
import numpy as np

F32, I32, F64 = np.float32, np.int32, np.float64
DROP = 2e-4
GRIDS = [(3, 4, 5), (12, 12, 12), (40, 40, 8)]
P = 700
CLUSTER = np.arange(252, 261)                      # nine points of one voxel, indices on both sides of the tile boundary 256


def _local(pts, box):
    """float64 local coordinates of pts (n, 3) in box (7)"""
    d = pts[:, :3].astype(F64) - box[:3].astype(F64)
    c, s = np.cos(-F64(box[6])), np.sin(-F64(box[6]))
    return np.stack([d[:, 0] * c - d[:, 1] * s, d[:, 0] * s + d[:, 1] * c, d[:, 2]], 1)


def _world(local, box):
    c, s = np.cos(F64(box[6])), np.sin(F64(box[6]))
    return np.stack([local[:, 0] * c - local[:, 1] * s, local[:, 0] * s + local[:, 1] * c, local[:, 2]], 1) + box[:3].astype(F64)


def _fragile(pts, boxes):
    """(in-box pairs (n, N) bool, fragile pairs (n, N) bool) evaluated in float64"""
    inside, frag = [], []
    for b in boxes:
        l, half = _local(pts, b), b[3:6].astype(F64) / 2
        ins = (np.abs(l) <= half + 1e-5).all(1)
        near = (np.abs(np.abs(l) - half) < DROP).any(1) | (np.abs(np.abs(l[:, :2]) - half[:2] - 1e-5) < DROP).any(1)
        near &= (np.abs(l) <= half + 2 * DROP).all(1)              # a face plane far outside the box decides nothing
        for grid in GRIDS:
            q = (l + half) / (2 * half / np.array(grid, F64))     # voxel coordinate; boundaries at the integers
            near |= ins & (np.abs(q - np.round(q)) * (2 * half / np.array(grid, F64)) < DROP).any(1)
        inside.append(ins)
        frag.append(near)
    return np.stack(inside, 1), np.stack(frag, 1)


def roiaware_inputs(kind, seed=7):
    """-> dict rois (6, 7), pts (700, 3), feat70 (700, 70), feat3 (700, 3), drop (share of the in-box pairs dropped)"""
    rng = np.random.default_rng(seed + (0 if kind == "exact" else 100))
    exact = kind == "exact"
    head = (lambda: 0.0) if exact else (lambda: rng.uniform(-np.pi, np.pi))
    rois = np.array([
        [30.0, 30.0, 1.0, 3.0, 4.0, 5.0, head()],                  # 0: empty, nothing near it
        [-10.0, 5.0, 0.0, 3.0, 4.0, 5.0, head()],                  # 1 and 2 overlap and share points
        [-9.0, 6.0, 0.5, 4.5, 3.0, 2.5, head()],
        [8.0, -12.0, -1.0, 6.0, 2.0, 3.0, 0.0 if exact else 0.7],  # 3: rotated
        [2.0, 20.0, 0.0, 1.5, 2.0, 2.5, 0.0],                      # 4: holds the cluster
        [-35.0, -37.0, 2.0, 3.0, 4.0, 5.0, head()],                # 5: far from the origin
    ], F32)
    if not exact:
        rois[4, 3:6] = [1.2, 1.6, 2.0]
    cand = []
    for b in (1, 2, 3, 5):
        n = 110
        if exact:
            half8 = (rois[b, 3:6] * 4).astype(int)                 # half extents in lattice steps
            l = np.stack([rng.integers(-h - 2, h + 3, n) for h in half8], 1) / 8.0   # faces and outside included
        else:
            l = rng.uniform(-0.56, 0.56, (n, 3)) * rois[b, 3:6]
        cand.append(_world(l, rois[b]))
    lo = rng.integers(-320, 321, (300, 3)) / 8.0 if exact else rng.uniform(-40, 40, (300, 3))
    lo[:, 2] = rng.integers(-32, 33, 300) / 8.0 if exact else lo[:, 2] / 10
    cand.append(lo)                                                # background
    cand = np.concatenate(cand).astype(F32)
    if exact:
        cluster = np.repeat((rois[4, :3] + np.array([-0.5, 0.25, 0.375], F32))[None], 9, 0)
    else:                                                          # the middle of one voxel of every grid, jitter 2 mm
        cluster = rois[4, :3] - rois[4, 3:6] / 2 + np.array([0.215, 0.46, 0.9], F32) + rng.uniform(-2e-3, 2e-3, (9, 3))
    cluster = cluster.astype(F32)
    drop = 0.0
    if not exact:
        ins, frag = _fragile(cand, rois)
        bad = frag.any(1)
        drop = float((ins & bad[:, None]).sum()) / max(int(ins.sum()), 1)
        assert drop <= 0.05, "the generator may drop at most 5 %% of the in-box pairs, not %.1f %%" % (100 * drop)
        cand = cand[~bad]
        assert not _fragile(cluster, rois)[1].any()
    cand = cand[rng.permutation(len(cand))[:P - 9]]
    assert len(cand) == P - 9
    pts = np.concatenate([cand[:CLUSTER[0]], cluster, cand[CLUSTER[0]:]]).astype(F32)
    feat70 = rng.normal(size=(P, 70)).astype(F32)
    feat70[CLUSTER[1]] = feat70[CLUSTER[3]] = np.abs(feat70[CLUSTER].max(0)) + 1   # a tie of two maxima: the lower slot wins
    return dict(rois=rois, pts=pts, feat70=feat70, feat3=np.ascontiguousarray(feat70[:, :3]), drop=drop)


def roipoint_inputs(kind, seed=11):
    """-> dict xyz (2, 700, 3), boxes (2, 5, 7), feat130 (2, 700, 130), feat5; counts (2, 5) of the plain boxes and
    counts_wide (2, 5) of the boxes enlarged by 1.0.  Boxes per scene: A (512 points), B (16 in scene 0, 7 in scene 1),
    C (20, ten of them with an index below 256 and ten above), E (contains A and 28 more: 540) and Z (empty; in scene 0
    three points sit 0.25 m outside its faces and fall into the enlarged box)."""
    rng = np.random.default_rng(seed + (0 if kind == "exact" else 100))
    exact = kind == "exact"
    xyz, boxes = np.zeros((2, P, 3), F32), np.zeros((2, 5, 7), F32)
    counts, counts_wide = np.zeros((2, 5), int), np.zeros((2, 5), int)
    for s in range(2):
        head = (lambda: 0.0) if exact else (lambda: rng.uniform(-np.pi, np.pi))
        A = np.array([-20, -20, 0, 4, 4, 2, head()], F32)
        E = np.array([-20, -20, 0, 8, 8, 3, A[6]], F32)            # same heading: A and the ring D around it
        B = np.array([10, 15, 1, 2, 3, 2, head()], F32)
        C = np.array([25, -10, -1, 3, 2, 2, head()], F32)
        Z = np.array([0, 0, 0, 2, 2, 2, head()], F32)
        boxes[s] = [A, B, C, E, Z]

        def inside(box, n, frac=0.45):
            if exact:
                h8 = np.floor(box[3:6] * 4).astype(int)
                l = np.stack([rng.integers(-h, h + 1, n) for h in h8], 1) / 8.0     # faces included: |l| == d / 2 is inside
            else:
                l = rng.uniform(-frac, frac, (n, 3)) * box[3:6]
            return _world(l, box)
        nB = 16 if s == 0 else 7
        groups = {"A": inside(A, 512), "B": inside(B, nB), "C": inside(C, 20)}
        ring = rng.uniform(-0.45, 0.45, (28, 3)) * E[3:6]
        ring[:, 0] = np.where(ring[:, 0] > 0, 1, -1) * rng.uniform(2.875, 3.5, 28)  # |x| in [2.875, 3.5]: outside A even enlarged
        if exact:
            ring = np.round(ring * 8) / 8
        groups["D"] = _world(ring, E)
        shell = np.array([[1.25, 0, 0], [0, -1.25, 0.5], [-1.25, 0.5, -0.5]], F64)  # 0.25 m outside Z, inside Z + 1.0
        groups["S"] = _world(shell, Z) if s == 0 else np.zeros((0, 3))
        n_bg = P - sum(len(g) for g in groups.values())
        bg = np.stack([rng.integers(320, 480, n_bg) / 8.0, rng.integers(-320, 320, n_bg) / 8.0, rng.integers(-8, 9, n_bg) / 8.0], 1)
        if not exact:
            bg = bg + rng.uniform(0, 0.1, bg.shape)
        groups["bg"] = bg                                          # x >= 40: away from every box
        perm = rng.permutation(P)
        low, high = perm[perm < 256], perm[perm >= 256]
        idx_c = np.concatenate([low[:10], high[:10]])
        rest = np.concatenate([low[10:], high[10:]])
        rest = rest[rng.permutation(len(rest))]
        xyz[s, idx_c] = groups["C"]
        at = 0
        for name in ("A", "B", "D", "S", "bg"):
            g = groups[name]
            xyz[s, rest[at:at + len(g)]] = g
            at += len(g)
        assert at == len(rest)
        for w, out in ((0.0, counts), (1.0, counts_wide)):
            for m in range(5):
                box = boxes[s, m].copy()
                box[3:6] += F32(w)
                l, half = _local(xyz[s], box), box[3:6].astype(F64) / 2
                near, within = np.abs(np.abs(l) - half) < 0.04, np.abs(l) <= half + 0.04
                for k in range(3):                                 # a face decides only where the other two axes are inside
                    others = within[:, [j for j in range(3) if j != k]].all(1)
                    assert exact or not (near[:, k] & others).any(), "a point too close to a face"
                out[s, m] = int((np.abs(l) <= half + 1e-5).all(1).sum())
        assert counts[s].tolist() == [512, nB, 20, 540, 0] and counts_wide[s].tolist() == [512, nB, 20, 540, 3 if s == 0 else 0]
    feat130 = rng.normal(size=(2, P, 130)).astype(F32)
    return dict(xyz=xyz, boxes=boxes, feat130=feat130, feat5=np.ascontiguousarray(feat130[..., :5]), counts=counts,
                counts_wide=counts_wide)
