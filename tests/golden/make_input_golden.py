#!/usr/bin/env python
"""Generates tests/golden/input_stage.npz: the REFERENCE's input stage
(pcdet/datasets/processor/data_processor.py DataProcessor: mask_points_and_boxes_outside_range ->
sample_points -> shuffle_points, then pcdet/datasets/dataset.py DatasetTemplate.collate_batch) run on synthetic ragged
scenes, with every draw it makes recorded:
  * np.random.choice -> `pick`, stored as RANKS into the array it picks from (near_idxs / arange(n), both ascending);
  * np.random.shuffle (sample_points) -> `perm1`: the permutation the shuffle applied (shuffled[t] = before[perm1[t]]),
    obtained by shuffling arange(len) with the same generator state -- Fisher-Yates swaps depend on the length only;
  * np.random.permutation (shuffle_points) -> `perm2`.
Absent modules are stubbed (reference_loader.py): skimage, SharedArray, cumm, roiaware_pool3d_cuda (box_utils imports it, the
range mask does not reach it), and dataset.py's augmentor / point-feature-encoder imports.  Only inputs and outputs are stored.

Box corners are kept 1e-4 or more away from every range plane: the reference rotates them through torch's CPU matmul,
whose rounding (summation order, FMA use) is not specified, so a corner closer to a plane than that could fall on
either side of it.

Run with the reference checkout:  python tests/golden/make_input_golden.py /path/to/reference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from reference_loader import cpu_torch, load, q as _q, reference_root  # noqa: E402
from pdanet_amd.config import AttrDict as AD  # noqa: E402

OUT = os.path.join(HERE, "input_stage.npz")
K = 4096
ONCE_RANGE = [-75.2, -75.2, -5.0, 75.2, 75.2, 3.0]
KITTI_RANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]


def import_reference(root):
    cpu_torch()
    stubs = {"ops.roiaware_pool3d.roiaware_pool3d_cuda": {}, "datasets.augmentor.data_augmentor": {"DataAugmentor": None},
             "datasets.processor.point_feature_encoder": {"PointFeatureEncoder": None}}
    dp, ds = load(root, "pcdet", ["datasets.processor.data_processor", "datasets.dataset"], stubs=stubs, real_paths=True)
    return dp.DataProcessor, ds.DatasetTemplate.collate_batch


class Recorder:
    """Wraps np.random.choice / shuffle / permutation; the draws of the current scene land in self.pick/perm1/perm2."""

    def __init__(self):
        self.choice, self.shuffle, self.permutation = np.random.choice, np.random.shuffle, np.random.permutation
        self.reset()

    def reset(self):
        self.pick, self.perm1, self.perm2 = np.zeros(0, np.int32), None, None

    def __enter__(self):
        rec = self

        def choice(a, size=None, replace=True, p=None):
            out = rec.choice(a, size, replace, p)
            a = np.asarray(a)
            assert np.all(np.diff(a) > 0)
            rec.pick = np.searchsorted(a, out).astype(np.int32)
            return out

        def shuffle(x):
            p = np.arange(len(x))
            rec.shuffle(p)
            x[:] = x[p].copy()
            rec.perm1 = p.astype(np.int32)

        def permutation(n):
            out = rec.permutation(n)
            rec.perm2 = out.astype(np.int32)
            return out

        np.random.choice, np.random.shuffle, np.random.permutation = choice, shuffle, permutation
        return self

    def __exit__(self, *a):
        np.random.choice, np.random.shuffle, np.random.permutation = self.choice, self.shuffle, self.permutation


# ---- synthetic scenes ----------------------------------------------------------------------------------------------------
def _cloud(rng, n, rmin, rmax, rng_xy, c, z=(-2.0, 0.5)):
    """n points at horizontal distance [rmin, rmax) from the origin inside the xy box rng_xy (x0, y0, x1, y1)."""
    out = np.zeros((0, c), np.float32)
    while out.shape[0] < n:
        m = 4 * n
        r = np.sqrt(rng.uniform(rmin ** 2, rmax ** 2, m))
        a = rng.uniform(-np.pi, np.pi, m)
        x, y = r * np.cos(a), r * np.sin(a)
        ok = (x > rng_xy[0] + 0.01) & (x < rng_xy[2] - 0.01) & (y > rng_xy[1] + 0.01) & (y < rng_xy[3] - 0.01)
        p = np.zeros((int(ok.sum()), c), np.float32)
        p[:, 0], p[:, 1] = _q(x[ok]), _q(y[ok])
        p[:, 2] = _q(rng.uniform(z[0], z[1], p.shape[0]))
        p[:, 3:] = _q(rng.uniform(0, 1, (p.shape[0], c - 3)))
        out = np.concatenate([out, p])
    return out[:n]


def _outside(rng, n, pr, c):
    """n points with x or y outside the range (z anything)."""
    p = np.zeros((n, c), np.float32)
    side = rng.integers(0, 4, n)
    p[:, 0] = _q(rng.uniform(pr[0], pr[3], n))
    p[:, 1] = _q(rng.uniform(pr[1], pr[4], n))
    p[side == 0, 0] = _q(pr[0] - rng.uniform(0.5, 20, (side == 0).sum()))
    p[side == 1, 0] = _q(pr[3] + rng.uniform(0.5, 20, (side == 1).sum()))
    p[side == 2, 1] = _q(pr[1] - rng.uniform(0.5, 20, (side == 2).sum()))
    p[side == 3, 1] = _q(pr[4] + rng.uniform(0.5, 20, (side == 3).sum()))
    p[:, 2] = _q(rng.uniform(-10, 10, n))
    p[:, 3:] = _q(rng.uniform(0, 1, (n, c - 3)))
    return p


def _sphere(rng, n, c, xpos):
    """n points within 2e-5 m of the 40 m sphere (both sides), x > 0 when xpos."""
    v = rng.normal(size=(n, 3))
    v[:, 2] *= 0.05
    if xpos:
        v[:, 0] = np.abs(v[:, 0]) + 0.3
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r = 40.0 + rng.uniform(-2e-5, 2e-5, n)
    p = np.zeros((n, c), np.float32)
    p[:, :3] = (v * r[:, None]).astype(np.float32)
    p[:, 3:] = _q(rng.uniform(0, 1, (n, c - 3)))
    return p


def _limits(pr, c):
    """points exactly on the x and y limits, and one float step outside them."""
    f = np.float32
    lo_x, lo_y, hi_x, hi_y = f(pr[0]), f(pr[1]), f(pr[3]), f(pr[4])
    mid_x, mid_y = f(0.5 * (pr[0] + pr[3]) + 0.25), f(0.5 * (pr[1] + pr[4]) + 0.25)
    rows = [(lo_x, mid_y), (hi_x, mid_y), (mid_x, lo_y), (mid_x, hi_y), (lo_x, lo_y), (hi_x, hi_y),
            (np.nextafter(lo_x, f(-1e9)), mid_y), (np.nextafter(hi_x, f(1e9)), mid_y),
            (mid_x, np.nextafter(lo_y, f(-1e9))), (mid_x, np.nextafter(hi_y, f(1e9)))]
    p = np.zeros((len(rows), c), np.float32)
    for i, (x, y) in enumerate(rows):
        p[i, 0], p[i, 1], p[i, 2] = x, y, f(pr[5] + 3.0 if i % 2 else pr[2] - 3.0)   # z outside: not tested
        p[i, 3:] = f(0.5)
    return p


def _corners(b):
    t = np.array([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]]) / 2.0
    loc = b[None, 3:6] * t
    c, s = np.cos(b[6]), np.sin(b[6])
    x = loc[:, 0] * c - loc[:, 1] * s
    y = loc[:, 0] * s + loc[:, 1] * c
    return np.stack([x, y, loc[:, 2]], 1) + b[None, 0:3]


def _boxes(rng, n, pr, kind):
    """kind 'mixed': inside, partly inside, outside; 'outside': all outside.  Corners >= 1e-4 from every plane."""
    out = []
    lo, hi = np.array(pr[:3]), np.array(pr[3:])
    while len(out) < n:
        dims = rng.uniform([1.5, 0.6, 1.4], [5.0, 2.5, 2.0])
        h = rng.uniform(-np.pi, np.pi)
        want = "outside" if kind == "outside" else ["inside", "partial", "outside"][len(out) % 3]
        if want == "inside":
            ctr = rng.uniform(lo + [4, 4, 0], hi - [4, 4, 0])
        else:
            ctr = rng.uniform(lo + [1, 1, 0], hi - [1, 1, 0])
            ax = rng.integers(0, 2)
            edge = lo[ax] if rng.integers(0, 2) == 0 else hi[ax]
            ctr[ax] = edge + rng.uniform(-1.0, 1.0) if want == "partial" else edge + np.sign(edge - ctr[ax] + 1e-9) * rng.uniform(4, 9)
        ctr[2] = rng.uniform(lo[2] + 1.2, hi[2] - 1.2)
        b = np.concatenate([ctr, dims, [h, rng.integers(1, 4)]]).astype(np.float32)
        cor = _corners(b.astype(np.float64))
        if np.min(np.abs(cor[:, :, None] - np.stack([lo, hi], 1)[None])) < 1e-4:
            continue
        inside = ((cor >= lo) & (cor <= hi)).all(1).sum()
        if (want == "inside" and inside != 8) or (want == "partial" and not 0 < inside < 8) or (want == "outside" and inside):
            continue
        out.append(b)
    return np.stack(out)


def scenes_once(rng):
    c, pr = 4, ONCE_RANGE
    xy = (pr[0], pr[1], pr[3], pr[4])
    s = []
    # case A: near + far + limit points + points on the 40 m sphere, partly-inside boxes
    s.append(np.concatenate([_cloud(rng, 3600, 1, 39.9, xy, c), _cloud(rng, 900, 40.1, 74, xy, c), _sphere(rng, 400, c, False),
                             _limits(pr, c), _outside(rng, 300, pr, c)]))
    # case B: at least K far points
    s.append(np.concatenate([_cloud(rng, 300, 1, 39, xy, c), _cloud(rng, 4300, 41, 74, xy, c), _outside(rng, 100, pr, c)]))
    # case C (padding), every box outside
    s.append(np.concatenate([_cloud(rng, 1500, 1, 39, xy, c), _cloud(rng, 800, 41, 70, xy, c), _outside(rng, 200, pr, c)]))
    boxes = [_boxes(rng, 9, pr, "mixed"), _boxes(rng, 5, pr, "mixed"), _boxes(rng, 4, pr, "outside")]
    return c, pr, s, boxes


def scenes_kitti(rng):
    c, pr = 5, KITTI_RANGE
    xy = (pr[0], pr[1], pr[3], pr[4])
    s = []
    # case A with no far point (everything within 40 m) + sphere points inside the sphere only
    sph = _sphere(rng, 300, c, True)
    sph = sph[np.linalg.norm(sph[:, :3], axis=1) < 40.0]
    s.append(np.concatenate([_cloud(rng, 4400, 1, 39.9, xy, c), sph, _outside(rng, 150, pr, c)]))
    # n == K exactly, with limit points among them
    lim = _limits(pr, c)
    n_in_lim = int(((lim[:, 0] >= np.float32(pr[0])) & (lim[:, 0] <= np.float32(pr[3])) & (lim[:, 1] >= np.float32(pr[1]))
                    & (lim[:, 1] <= np.float32(pr[4]))).sum())
    s.append(np.concatenate([_cloud(rng, K - 300 - n_in_lim, 1, 39, xy, c), _cloud(rng, 300, 41, 70, xy, c), lim,
                             _outside(rng, 250, pr, c)]))
    # most points outside the range (padding case)
    s.append(np.concatenate([_outside(rng, 4200, pr, c), _cloud(rng, 1800, 1, 60, xy, c)]))
    boxes = [_boxes(rng, 6, pr, "mixed"), _boxes(rng, 3, pr, "mixed"), _boxes(rng, 7, pr, "mixed")]
    return c, pr, s, boxes


def run(DataProcessor, collate, c, pr, scenes, boxes, training, seed):
    cfg = [AD(NAME="mask_points_and_boxes_outside_range", REMOVE_OUTSIDE_BOXES=True),
           AD(NAME="sample_points", NUM_POINTS=AD(train=K, test=K)),
           AD(NAME="shuffle_points", SHUFFLE_ENABLED=AD(train=True, test=False))]
    dp = DataProcessor(cfg, np.array(pr, np.float32), training, c)
    np.random.seed(seed)
    perm = lambda s: s[np.random.permutation(len(s))]    # noqa: E731  (scenes arrive in sensor order)
    scenes = [perm(s) for s in scenes]
    rec = Recorder()
    outs, draws = [], {"pick": [], "perm1": [], "perm2": []}
    with rec:
        for pts, bx in zip(scenes, boxes):
            rec.reset()
            d = dp.forward({"points": pts.copy(), "gt_boxes": bx.copy()})
            outs.append(d)
            draws["pick"].append(rec.pick)
            draws["perm1"].append(rec.perm1)
            draws["perm2"].append(rec.perm2 if training else np.zeros(0, np.int32))
    batch = collate(outs)
    return scenes, batch, draws


def main():
    DataProcessor, collate = import_reference(reference_root())
    rng = np.random.default_rng(20261016)
    data, cases = {}, []
    for tag, maker, training, seed in (("once", scenes_once, True, 11), ("kitti", scenes_kitti, False, 12)):
        c, pr, scenes, boxes = maker(rng)
        scenes, batch, draws = run(DataProcessor, collate, c, pr, scenes, boxes, training, seed)
        B = len(scenes)
        data[tag + "_range"] = np.array(pr, np.float32)
        data[tag + "_training"] = np.array(training)
        data[tag + "_points_raw"] = np.concatenate(scenes)
        data[tag + "_offsets"] = np.concatenate([[0], np.cumsum([len(s) for s in scenes])]).astype(np.int64)
        data[tag + "_boxes_raw"] = np.concatenate(boxes)
        data[tag + "_box_offsets"] = np.concatenate([[0], np.cumsum([len(b) for b in boxes])]).astype(np.int64)
        for key in ("pick", "perm1", "perm2"):
            data[tag + "_" + key] = np.concatenate(draws[key]).astype(np.int32)
            data[tag + "_" + key + "_offsets"] = np.concatenate([[0], np.cumsum([len(x) for x in draws[key]])]).astype(np.int64)
        data[tag + "_ref_points"] = batch["points"].astype(np.float32)
        data[tag + "_ref_gt_boxes"] = batch["gt_boxes"].astype(np.float32)
        kept = [int((np.abs(batch["gt_boxes"][b]).sum(1) > 0).sum()) for b in range(B)]
        data[tag + "_ref_kept"] = np.array(kept, np.int32)
        cases.append((tag, [len(s) for s in scenes], [len(x) for x in draws["pick"]], kept))
    data["num_points"] = np.array(K)
    np.savez_compressed(OUT, **data)
    for cse in cases:
        print("%s: raw sizes %s, picks %s, kept boxes %s" % cse)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
