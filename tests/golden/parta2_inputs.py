"""Seeded inputs of the Part-A2 tests (tests/test_part_head.py, tests/test_parta2_head.py) and of make_parta2_golden.py, with
the plain statements the tests hold the kernels of csrc/parta2.hip against.

part_head_inputs: two scenes of 300 and 173 points (ragged) and four ground-truth boxes each: two that overlap, two apart; in
scene 1 the last row is zero-padded.  Points are drawn in the boxes' frames so that each scene holds points inside a box,
points inside an enlarged box only (GT_EXTRA_WIDTH 0.2) and points outside both; three points of scene 1 lie inside the
enlarged zero row at the origin, which the reference labels -1 like any other.  Every candidate within MARGIN = 1e-3 m of a
face plane of any box of its scene, plain or enlarged, evaluated in float64 on the float32 coordinates, is dropped: coordinates
below 64 m have a float32 ulp of 3.8e-6 m and a local coordinate accumulates fewer than five roundings, so no label depends on
the arithmetic (label_statement in float32 and in float64 agree; the tests assert it).

pool_inputs: two scenes of 500 and 300 points with 16 feature channels, part offsets in (0, 1), scores in (0, 1) on both sides
of SEG_MASK_SCORE_THRESH = 0.3, and three RoIs per scene: scene 0 holds two overlapping RoIs and an empty one, scene 1 two RoIs
and a zero-padded row.  A cluster of 12 points sits in one voxel of the 12^3 grid, so with MAX_POINTS_PER_VOXEL = 8 voxels
overflow their 7 slots.  Candidates near a box face or a voxel boundary of the 12^3 grid (which holds the 4^3 one's) are
dropped by roi_pool_inputs._fragile, so no decision depends on the contraction mode."""
import numpy as np

import roi_pool_inputs as rp

F32, F64 = np.float32, np.float64
MARGIN = 1e-3
EXTRA_WIDTH = (0.2, 0.2, 0.2)
PART_COUNTS = (300, 173)
POOL_COUNTS = (500, 300)
POOL_CHANNELS = 16
POOL_THRESH = 0.3
POOL_K = 8


def _planes_clear(pts, boxes, extra):
    """True for the points at least MARGIN from every face plane of every box, plain and enlarged (float64)."""
    ok = np.ones(len(pts), bool)
    for b in boxes.astype(F64):
        l = rp._local(pts, b.astype(F32))
        for half in (b[3:6] / 2, (b[3:6] + np.asarray(extra, F64)) / 2):
            ok &= (np.abs(np.abs(l) - half) >= MARGIN).all(1)
    return ok


def part_head_inputs(seed=3):
    """-> dict points (473, 4) float32 [bs, x, y, z] scene-major, gt_boxes (2, 4, 8) float32, extra_width, counts."""
    rng = np.random.default_rng(seed)
    gt = np.zeros((2, 4, 8), F32)
    gt[0] = [[10.0, 2.0, -0.5, 3.9, 1.6, 1.5, 0.4, 1], [11.0, 2.5, -0.4, 4.2, 1.8, 1.6, -0.9, 2],      # 0 and 1 overlap
             [25.0, -8.0, -0.8, 0.8, 0.6, 1.7, 2.1, 2], [18.0, 10.0, -0.6, 1.8, 0.6, 1.7, -2.6, 3]]
    gt[1] = [[8.0, -3.0, -0.7, 3.6, 1.5, 1.4, -0.3, 1], [8.5, -2.0, -0.6, 1.7, 0.7, 1.8, 1.2, 3],       # 0 and 1 overlap
             [30.0, 12.0, -0.9, 4.1, 1.7, 1.6, 3.0, 1], [0, 0, 0, 0, 0, 0, 0, 0]]                       # a zero-padded row
    extra = np.asarray(EXTRA_WIDTH, F64)
    scenes = []
    for s, total in enumerate(PART_COUNTS):
        cand = []
        for b in gt[s]:
            if b[3] == 0:
                continue
            half = b[3:6].astype(F64) / 2
            inside = rng.uniform(-1, 1, (40, 3)) * (half - 0.01)
            ring = rng.uniform(-1, 1, (24, 3)) * (half + 0.09)
            axis = rng.integers(0, 3, 24)
            ring[np.arange(24), axis] = rng.choice([-1, 1], 24) * (half[axis] + rng.uniform(0.01, 0.09, 24))
            cand += [rp._world(inside, b), rp._world(ring, b)]
        if s == 1:
            cand.append(rng.choice([-1, 1], (3, 3)) * rng.uniform(0.03, 0.07, (3, 3)))                  # in the enlarged zero row only
        bg = np.stack([rng.uniform(0, 40, 400), rng.uniform(-20, 20, 400), rng.uniform(-2, 1, 400)], 1)
        cand = np.concatenate(cand + [bg]).astype(F32)
        cand = cand[_planes_clear(cand, gt[s], extra)]
        origin = np.abs(cand).max(1) < 0.1                                                               # always kept (scene 1 only)
        rest = rng.permutation(np.nonzero(~origin)[0])[:total - int(origin.sum())]
        pts = cand[rng.permutation(np.concatenate([np.nonzero(origin)[0], rest]))]
        assert len(pts) == total
        scenes.append(np.concatenate([np.full((total, 1), s, F32), pts], 1))
    return dict(points=np.concatenate(scenes).astype(F32), gt_boxes=gt, extra_width=EXTRA_WIDTH, counts=PART_COUNTS)


def label_statement(points, gt_boxes, extra_width, dtype, single_class):
    """assign_stack_targets(set_ignore_flag=True, ret_part_labels=True) stated point by point in `dtype`: the first box that
    holds the point gives label and part label, a point in an enlarged box only is -1.  -> labels (P) int64, part (P, 3) dtype."""
    pts, gt = np.asarray(points).astype(dtype), np.asarray(gt_boxes).astype(dtype)
    extra, margin = np.asarray(extra_width).astype(dtype), dtype(1e-5)
    labels, part = np.zeros(len(pts), np.int64), np.zeros((len(pts), 3), dtype)
    for i, row in enumerate(pts):
        s = int(row[0])
        if not (0 <= s < len(gt)) or dtype(s) != row[0]:
            continue
        ib = ie = -1
        for k, b in enumerate(gt[s]):
            a = -b[6]
            c, sn = np.cos(a), np.sin(a)
            d = row[1:4] - b[0:3]
            loc = np.array([d[0] * c + d[1] * (-sn), d[0] * sn + d[1] * c, d[2]], dtype)
            for which, dims in enumerate((b[3:6], b[3:6] + extra)):
                hit = abs(loc[2]) <= dims[2] / 2 and abs(loc[0]) < dims[0] / 2 + margin and abs(loc[1]) < dims[1] / 2 + margin
                if hit and which == 0 and ib < 0:
                    ib = k
                    labels[i] = 1 if single_class else int(b[7])
                    part[i] = loc / b[3:6] + dtype(0.5)
                if hit and which == 1 and ie < 0:
                    ie = k
        if ib < 0 and ie >= 0:
            labels[i] = -1
    return labels, part


def pool_inputs(seed=9):
    """-> dict rois (2, 3, 7), point_coords (800, 4) [bs, x, y, z] scene-major, point_features (800, 16), point_part_offset
    (800, 3), point_cls_scores (800), counts, thresh, k_slots."""
    rng = np.random.default_rng(seed)
    rois = np.zeros((2, 3, 7), F32)
    rois[0] = [[12.0, 3.0, -0.5, 3.9, 1.6, 1.5, 0.5], [12.6, 3.3, -0.4, 4.1, 1.8, 1.7, -0.4],          # overlap and share points
               [35.0, -15.0, 0.0, 3.0, 1.5, 1.5, 1.0]]                                                  # empty
    rois[1] = [[20.0, -6.0, -0.6, 3.7, 1.6, 1.6, 2.2], [9.0, 9.0, -0.8, 1.2, 1.6, 2.0, -1.3], [0, 0, 0, 0, 0, 0, 0]]
    scenes, cluster_at = [], None
    for s, total in enumerate(POOL_COUNTS):
        cand = []
        live = [b for b in rois[s] if b[3] > 0 and not (s == 0 and b[0] == 35.0)]
        for b in live:
            cand.append(rp._world(rng.uniform(-0.56, 0.56, (160, 3)) * b[3:6].astype(F64), b))
        cand.append(np.stack([rng.uniform(4, 38, 300), rng.uniform(-12, 12, 300), rng.uniform(-2, 1, 300)], 1))
        cand = np.concatenate(cand).astype(F32)
        keepable = ~rp._fragile(cand, rois[s][rois[s][:, 3] > 0])[1].any(1)
        far = (np.abs(cand[:, :2] - np.array([35.0, -15.0], F32)) > 4).any(1) if s == 0 else np.abs(cand).max(1) > 1.0
        cand = cand[keepable & far]
        n_cluster = 12 if s == 1 else 0
        pts = cand[rng.permutation(len(cand))[:total - n_cluster]]
        if s == 1:                                                   # twelve points in the middle of one voxel of the 12^3 grid
            b = rois[1, 1]
            cell = b[3:6].astype(F64) / 12
            centre = -b[3:6].astype(F64) / 2 + (np.array([4, 7, 5]) + 0.5) * cell
            cluster = rp._world(centre + rng.uniform(-0.2, 0.2, (12, 3)) * cell, b).astype(F32)
            assert not rp._fragile(cluster, rois[1][:2])[1].any()
            pts = np.concatenate([pts[:250], cluster, pts[250:]])     # indices on both sides of the tile boundary 256
        assert len(pts) == total
        scenes.append(np.concatenate([np.full((total, 1), s, F32), pts], 1))
    coords = np.concatenate(scenes).astype(F32)
    n = len(coords)
    return dict(rois=rois, point_coords=coords, point_features=rng.normal(size=(n, POOL_CHANNELS)).astype(F32),
                point_part_offset=rng.uniform(0.02, 0.98, (n, 3)).astype(F32),
                point_cls_scores=rng.uniform(0.01, 0.99, n).astype(F32), counts=POOL_COUNTS, thresh=POOL_THRESH, k_slots=POOL_K)
