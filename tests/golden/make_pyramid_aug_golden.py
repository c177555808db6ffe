#!/usr/bin/env python
"""Generates tests/golden/pyramid_aug.npz: the REFERENCE's random_local_pyramid_aug (augmentor_utils.py
local_pyramid_dropout -> local_pyramid_sparsify -> local_pyramid_swap, as data_augmentor.py chains them) on small synthetic
scenes, with every np.random draw it made and every output row traced to its input row.

The reference is read through make_augment_golden.import_reference(); nothing of it is stored: the fixture holds inputs,
draws, outputs and coverage counts.

Scenes (C = 4, SPARSIFY_MAX_NUM = SWAP_MAX_NUM = 8, probabilities 0.5): `main` about 1 500 points and six boxes, four of
150-300 points interleaved through the scene (every pyramid spans several 256-point tiles), two sparse ones (a
selected-but-not-thinned pyramid, a swap-selected box without a valid face), one of them of class 0 with points; `single`
one box (its swap partner is itself); `nobox`; `alldrop` a scene whose dropout selects every box.  Each is searched over
seeds until its coverage holds.

Tracing: np.random.randint / uniform / choice are wrapped and their results recorded in call order; points_in_pyramids_mask
is wrapped and its results kept.  The dropout and the sparsify only select rows, so their output rows are found in the input
by their bits (the xyz of a scene are distinct); the swap's output is remain_points, then per pair the partner's rows
rebuilt in the to-swap pyramid, then the to-swap rows rebuilt in the partner -- the recorded masks say which rows those are.
A self pair emits its pyramid's rows twice (rebuilt in their own frame): both copies are folded onto the input row and
flagged 2; a really swapped row is flagged 1.

Knife edges: a raw point that in float64 lies within 1e-4 of a face plane of a box or of a diagonal plane between two
of its pyramids is dropped before the run (make_augment_steps_golden.py's rule; the closed form and the reference's
Delaunay test may differ there).  Attempts with a contested partner pyramid are rejected; the boxes of a scene never overlap.

`paste` has gt_sampling in front: the reference's DataBaseSampler pastes objects of a synthetic database (dbinfos and
per-object point files in make_augment_golden's format, 90-160 points an object) into a scene with a class-0 box, and the three
functions run on what it leaves.  The fixture keeps the raw scene, the database, the candidates the sampler tried, the
pasted scene (the input of the step, stored under the keys of the other cases) and the step's draws and output; an attempt
is taken only when a pasted box is dropped or thinned and a pasted box is in a real swap.  Box pairs are robust against the
collision test (make_augment_golden._robust_pairs) and no raw point lies near a face of a database box.

Run with the reference checkout:  python tests/golden/make_pyramid_aug_golden.py /path/to/reference
"""
import os
import pathlib
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_augment_golden as mag  # noqa: E402
from make_augment_golden import import_reference  # noqa: E402
from reference_loader import reference_root  # noqa: E402
from pdanet_amd.config import to_attr  # noqa: E402

OUT = os.path.join(HERE, "pyramid_aug.npz")
CFG = dict(DROP_PROB=0.5, SPARSIFY_PROB=0.5, SPARSIFY_MAX_NUM=8, SWAP_PROB=0.5, SWAP_MAX_NUM=8)
f32 = np.float32


def _local(points, box):
    """float64 box-frame coordinates of the points."""
    p = np.asarray(points, np.float64)
    b = np.asarray(box, np.float64)
    c, s = np.cos(-b[6]), np.sin(-b[6])
    sx, sy = p[:, 0] - b[0], p[:, 1] - b[1]
    return np.stack([sx * c - sy * s, sx * s + sy * c, p[:, 2] - b[2]], 1)


def near_plane(points, boxes, tol=1e-4):
    bad = np.zeros(len(points), bool)
    for b in boxes:
        loc = np.abs(_local(points, b))
        h = np.asarray(b[3:6], np.float64) / 2
        close = (loc <= h + tol).all(1)
        face = (np.abs(loc - h) <= tol).any(1)
        diag = np.zeros(len(points), bool)
        for a, c in ((0, 1), (0, 2), (1, 2)):                       # |l_a| / h_a = |l_c| / h_c
            diag |= np.abs(loc[:, a] * h[c] - loc[:, c] * h[a]) / np.hypot(h[a], h[c]) <= tol
        bad |= close & (face | diag)
    return bad


def make_scene(rng, counts, n_bg):
    """Boxes on a grid (no overlap), counts[i] points inside box i, n_bg background points, interleaved."""
    m = len(counts)
    dims = np.array([(4.2, 1.8, 1.6), (0.8, 0.7, 1.7), (1.8, 0.7, 1.5), (7.0, 2.5, 2.8)])
    d = dims[rng.integers(0, 4, m)] * rng.uniform(0.9, 1.1, (m, 3))
    ctr = np.stack([10.0 + 12.0 * np.arange(m) + rng.uniform(-1, 1, m), rng.uniform(-20, 20, m), -1.6 + d[:, 2] / 2], 1)
    bx = np.concatenate([ctr, d, rng.uniform(-np.pi, np.pi, (m, 1))], 1).astype(f32)
    rows = []
    for i, k in enumerate(counts):
        loc = rng.uniform(-0.5, 0.5, (k, 3)) * bx[i, 3:6]
        c, s = np.cos(bx[i, 6]), np.sin(bx[i, 6])
        rows.append(np.stack([loc[:, 0] * c - loc[:, 1] * s + bx[i, 0], loc[:, 0] * s + loc[:, 1] * c + bx[i, 1], loc[:, 2] + bx[i, 2]], 1))
    rows.append(np.concatenate([rng.uniform([0, -30], [90, 30], (n_bg, 2)), rng.uniform(-2.5, 0.5, (n_bg, 1))], 1))
    xyz = np.concatenate(rows)[rng.permutation(sum(counts) + n_bg)]
    p = np.concatenate([xyz, rng.uniform(0, 1, (len(xyz), 1))], 1).astype(f32)
    p = p[~near_plane(p, bx)]
    _, first = np.unique(p[:, :3].view([("", f32)] * 3), return_index=True)
    return p[np.sort(first)], bx


class Recorder:
    """np.random.randint / uniform / choice and points_in_pyramids_mask, recorded in call order."""

    def __init__(self, au):
        self.au, self.events, self.masks = au, [], []

    def __enter__(self):
        self.saved = (np.random.randint, np.random.uniform, np.random.choice, self.au.points_in_pyramids_mask)

        def wrap(name, fn):
            def inner(*a, **k):
                r = fn(*a, **k)
                self.events.append((name, np.array(r)))
                return r
            return inner

        def mask(points, pyramids):
            r = self.saved[3](points, pyramids)
            self.masks.append(np.array(r))
            return r

        np.random.randint, np.random.uniform, np.random.choice = (wrap(n, f) for n, f in zip(("randint", "uniform", "choice"), self.saved))
        self.au.points_in_pyramids_mask = mask
        return self

    def __exit__(self, *a):
        np.random.randint, np.random.uniform, np.random.choice, self.au.points_in_pyramids_mask = self.saved


def _find(rows, base):
    """The row of `base` every row of `rows` is a bit copy of."""
    key = lambda a: [r.tobytes() for r in np.ascontiguousarray(a)]
    at = {k: i for i, k in enumerate(key(base))}
    assert len(at) == len(base)
    return np.array([at[k] for k in key(rows)], np.int64)


def run(au, points, boxes, seed):
    """-> None for a rejected attempt, else dict(draws, ref_points, ref_src, ref_flag, cover)."""
    np.random.seed(seed)
    m = len(boxes)
    cover = dict(dropped=0, thinned=0, selected_not_thinned=0, real_swap=0, self_swap=0, no_face=0)
    with Recorder(au) as rec:
        _, p1, pyr1 = au.local_pyramid_dropout(boxes.copy(), points.copy(), CFG["DROP_PROB"])
        n_ev1, n_mk1 = len(rec.events), len(rec.masks)
        _, p2, pyr2 = au.local_pyramid_sparsify(boxes.copy(), p1, CFG["SPARSIFY_PROB"], CFG["SPARSIFY_MAX_NUM"], pyr1)
        n_ev2, n_mk2 = len(rec.events), len(rec.masks)
        _, p3 = au.local_pyramid_swap(boxes.copy(), p2, CFG["SWAP_PROB"], CFG["SWAP_MAX_NUM"], pyr2)
    ev, mk = rec.events, rec.masks
    d = dict(drop_face=ev[0][1].astype(np.int32), drop_u=ev[1][1].astype(np.float64))
    cover["dropped"] = int((d["drop_u"] <= CFG["DROP_PROB"]).sum())
    L1 = len(pyr1)
    # sparsify: randint, uniform, then one choice per thinned pyramid in box order
    d.update(sparsify_face=np.zeros(0, np.int32), sparsify_u=np.zeros(0), sparsify_keep=[])
    if L1:
        d["sparsify_face"], d["sparsify_u"] = ev[n_ev1][1].astype(np.int32), ev[n_ev1 + 1][1].astype(np.float64)
        sel = d["sparsify_u"] <= CFG["SPARSIFY_PROB"]
        nums = mk[n_mk1].sum(0) if sel.any() else np.zeros(0, np.int64)
        choices = [e[1] for e in ev[n_ev1 + 2:n_ev2]]
        assert all(e[0] == "choice" for e in ev[n_ev1 + 2:n_ev2]) and len(choices) == int((nums > CFG["SPARSIFY_MAX_NUM"]).sum())
        keep, it = [np.zeros(0, np.int32)] * L1, iter(choices)
        for j, cnt in zip(np.nonzero(sel)[0], nums):
            if cnt > CFG["SPARSIFY_MAX_NUM"]:
                keep[j] = np.asarray(next(it), np.int32)
                cover["thinned"] += 1
            else:
                cover["selected_not_thinned"] += 1
        d["sparsify_keep"] = keep
    # swap: uniform, then a face choice per selected box with a valid face, then a partner choice per pair with a candidate
    L2 = len(pyr2)
    src2 = _find(p2, points)
    d.update(swap_u=ev[n_ev2][1].astype(np.float64), swap_face=np.full(L2, -1, np.int32), swap_partner=np.full(L2, -1, np.int32))
    assert len(d["swap_u"]) == L2
    sel = d["swap_u"] <= CFG["SWAP_PROB"]
    src, flag = src2, np.zeros(len(p2), np.int8)
    if sel.any():
        nums = mk[n_mk2].sum(0).reshape(L2, 6)
        valid = nums > CFG["SWAP_MAX_NUM"]
        rest = [e[1] for e in ev[n_ev2 + 1:]]
        boxes_sw = [k for k in range(L2) if sel[k] and valid[k].any()]
        cover["no_face"] = int(sel.sum()) - len(boxes_sw)
        if boxes_sw:
            fc = [int(x) for x in rest[:len(boxes_sw)]]
            for k, f in zip(boxes_sw, fc):
                d["swap_face"][k] = f
                valid[k, f] = False
            it = iter(rest[len(boxes_sw):])
            partners = []
            for k, f in zip(boxes_sw, fc):
                q = int(next(it)) if valid[:, f].any() else k
                partners.append(q)
                if q != k:
                    d["swap_partner"][k] = q
            assert next(it, None) is None
            if len({(q, f) for q, f in zip(partners, fc)}) < len(fc):
                return None                                          # a contested partner pyramid
            K = len(fc)
            sm = mk[-1]
            assert sm.shape == (len(p2), 2 * K)
            if (sm.sum(1) > 1).any() and any(q != k for q, k in zip(partners, boxes_sw)):
                own = sm[:, [i for i in range(K) if partners[i] != boxes_sw[i]] + [i + K for i in range(K) if partners[i] != boxes_sw[i]]]
                if (own.sum(1) > 1).any():
                    return None                                      # a point in two pyramids of real pairs
            rows, flags = [np.nonzero(~sm.any(1))[0]], [np.zeros(int((~sm.any(1)).sum()), np.int8)]
            for i in range(K):
                code = 2 if partners[i] == boxes_sw[i] else 1
                cover["self_swap" if code == 2 else "real_swap"] += 1
                for col in (i + K, i):
                    r = np.nonzero(sm[:, col])[0]
                    rows.append(r)
                    flags.append(np.full(len(r), code, np.int8))
            rows, flag = np.concatenate(rows), np.concatenate(flags)
            assert len(rows) == len(p3)
            src = src2[rows]
    assert len(src) == len(p3)
    assert np.array_equal(p3[flag == 0], points[src[flag == 0]])
    # fold the doubled rows of a self pair
    _, first = np.unique(src, return_index=True)
    first = np.sort(first)
    if len(first) < len(src):
        assert (flag[np.setdiff1d(np.arange(len(src)), first)] == 2).all()
    return dict(draws=d, ref_points=p3[first].astype(f32), ref_src=src[first], ref_flag=flag[first], cover=cover)


def search(au, rng, counts, n_bg, need, tries=400):
    for t in range(tries):
        p, bx = make_scene(rng, counts, n_bg)
        seed = int(rng.integers(0, 2 ** 31))
        r = run(au, p, bx, seed)
        if r is not None and need(r):
            print("  found after %d tries: %s, %d -> %d rows" % (t + 1, r["cover"], len(p), len(r["ref_points"])))
            return p, bx, r
    raise SystemExit("no attempt met the coverage")


CLASSES = ["Car", "Pedestrian", "Cyclist"]
GT_SAMPLING = {"NAME": "gt_sampling", "USE_ROAD_PLANE": False, "DB_INFO_PATH": ["dbinfos.pkl"],
               "PREPARE": {"filter_by_min_points": ["Car:5", "Pedestrian:5", "Cyclist:5"], "filter_by_difficulty": [-1]},
               "SAMPLE_GROUPS": ["Car:2", "Pedestrian:2", "Cyclist:1"], "NUM_POINT_FEATURES": 4, "DATABASE_WITH_FAKELIDAR": False,
               "REMOVE_EXTRA_WIDTH": [0.0, 0.0, 0.0], "LIMIT_WHOLE_SCENE": False}


def make_paste_db(rng):
    """dbinfos and point files as make_augment_golden.make_db writes them, with enough points an object for the step."""
    infos, bins = {}, {}
    dims = {"Car": (4.2, 1.8, 1.6), "Pedestrian": (0.8, 0.7, 1.7), "Cyclist": (1.8, 0.7, 1.5)}
    for name in CLASSES:
        lst = []
        for i in range(3):
            d = np.array(dims[name]) * rng.uniform(0.9, 1.1, 3)
            box = np.array([rng.uniform(5, 85), rng.uniform(-28, 28), -1.6 + d[2] / 2] + list(d) + [rng.uniform(-3.0, 3.0)], np.float64)
            n = int(rng.integers(90, 160))
            loc = rng.uniform(-0.45, 0.45, (n, 3)) * d
            x, y = mag._rot(loc[:, 0], loc[:, 1], box[6])
            pts = np.concatenate([np.stack([x, y, loc[:, 2]], 1), rng.uniform(0, 1, (n, 1))], 1).astype(f32)
            path = "gt_database/%s_%d.bin" % (name, i)
            bins[path] = pts
            lst.append({"name": name, "path": path, "box3d_lidar": box, "num_points_in_gt": n, "difficulty": 0, "gt_idx": i})
        infos[name] = lst
    return infos, bins


def paste_case(refs, au, iou_fn):
    """-> raw scene, database, candidates, the pasted scene and the step's run on it."""
    DataAugmentor = refs[0]
    for attempt in range(3000):
        rng = np.random.default_rng(7000 + attempt)
        infos, bins = make_paste_db(rng)
        p, bx = make_scene(rng, [220, 180, 40], 500)
        names = np.array(["Car", "Van", "Cyclist"], dtype="<U10")
        dbb = np.array([i["box3d_lidar"] for n in CLASSES for i in infos[n]])
        if not mag._robust_pairs(list(dbb) + list(bx), iou_fn):
            continue
        p = p[~mag._near_face(p, dbb, [0.0, 0.0, 0.0]) & ~near_plane(p, dbb)]
        for n in CLASSES:                                        # object points against their own pyramid planes
            for i in infos[n]:
                q = bins[i["path"]]
                w = q.copy()
                w[:, :3] = (q[:, :3].astype(np.float64) + i["box3d_lidar"][:3]).astype(f32)
                bins[i["path"]] = q[~near_plane(w, i["box3d_lidar"][None].astype(f32))]
                i["num_points_in_gt"] = len(bins[i["path"]])
        tmp = tempfile.mkdtemp()
        os.makedirs(os.path.join(tmp, "gt_database"))
        with open(os.path.join(tmp, "dbinfos.pkl"), "wb") as f:
            pickle.dump(infos, f)
        for path, q in bins.items():
            q.tofile(os.path.join(tmp, path))
        cfg = {"DISABLE_AUG_LIST": ["placeholder"], "AUG_CONFIG_LIST": [GT_SAMPLING, dict(CFG, NAME="random_local_pyramid_aug")]}
        aug = DataAugmentor(pathlib.Path(tmp), to_attr(cfg), CLASSES, logger=None)
        sampler = aug.data_augmentor_queue[0]
        gid, start, tried = {}, 0, []
        for n in CLASSES:
            for k, info in enumerate(sampler.db_infos[n]):
                gid[id(info)] = start + k
            start += len(sampler.db_infos[n])
        group_of = {n: g for g, n in enumerate(sampler.sample_groups)}
        orig = sampler.sample_with_fixed_number

        def swf(class_name, sample_group):
            out = orig(class_name, sample_group)
            tried.extend((gid[id(i)], group_of[class_name]) for i in out)
            return out
        sampler.sample_with_fixed_number = swf
        np.random.seed(attempt)
        d = sampler(data_dict={"points": p.copy(), "gt_boxes": bx.copy(), "gt_names": names.copy(),
                               "gt_boxes_mask": np.ones(len(bx), bool)})
        pp, pb, pn = d["points"].astype(f32), d["gt_boxes"].astype(f32), d["gt_names"]
        n_own, n_acc = len(bx), len(pb) - len(bx)
        if n_acc < 2 or n_acc == len(tried) or near_plane(pp, pb).any():
            continue
        if len(np.unique(pp[:, :3].view([("", f32)] * 3))) != len(pp):
            continue
        r = run(au, pp, pb, 100 + attempt)
        if r is None:
            continue
        dr = r["draws"]
        left1 = [i for i in range(len(pb)) if not dr["drop_u"][i] <= CFG["DROP_PROB"]]
        thinned = [left1[j] for j, k in enumerate(dr["sparsify_keep"]) if len(k)]
        left2 = [i for j, i in enumerate(left1) if not dr["sparsify_u"][j] <= CFG["SPARSIFY_PROB"]]
        swaps = [(left2[k], left2[q]) for k, q in enumerate(dr["swap_partner"]) if q >= 0]
        dropped = [i for i in range(len(pb)) if i not in left1]
        pasted = lambda i: i >= n_own
        if not (any(pasted(i) for i in dropped + thinned) and thinned and any(pasted(a) or pasted(q) for a, q in swaps)):
            continue
        if not any(pasted(a) != pasted(q) for a, q in swaps):            # a scene box and a pasted one change points
            continue
        print("  paste: attempt %d, %d candidates, %d accepted, dropped %s thinned %s swaps %s, %d -> %d -> %d rows" % (
            attempt, len(tried), n_acc, dropped, thinned, swaps, len(p), len(pp), len(r["ref_points"])))
        raw = dict(raw_points=p, raw_boxes=bx, raw_names=names, cand=np.array([t[0] for t in tried], np.int32),
                   cand_group=np.array([t[1] for t in tried], np.int32), n_accepted=np.array(n_acc, np.int32),
                   aug_cfg=np.array(pickle.dumps(cfg, protocol=4)), dbinfos=np.array(pickle.dumps(infos, protocol=4)),
                   db_paths=np.array(sorted(bins)), db_points=np.concatenate([bins[k] for k in sorted(bins)]),
                   db_point_offsets=np.concatenate([[0], np.cumsum([len(bins[k]) for k in sorted(bins)])]).astype(np.int64))
        return (pp, pb, r), pn, raw
    raise SystemExit("no paste attempt met the coverage")


def main():
    refs = import_reference(reference_root())
    import oracle

    def iou_fn(a, b):
        a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
        ans = np.zeros((a.shape[0], b.shape[0]), f32)
        oracle.boxes_overlap_bev_gpu(a, b, ans)
        return ans

    au = sys.modules["pcdet.datasets.augmentor.augmentor_utils"]
    rng = np.random.default_rng(20260321)
    cases = {}
    c = lambda r: r["cover"]
    print("main")
    cases["main"] = search(au, rng, [280, 240, 200, 160, 14, 30], 580,
                           lambda r: c(r)["dropped"] and c(r)["thinned"] and c(r)["selected_not_thinned"] and c(r)["real_swap"]
                           and c(r)["no_face"] and c(r)["dropped"] < 6)
    print("swap2 (two real pairs or more boxes left)")
    cases["swap2"] = search(au, rng, [260, 220, 200, 180, 150, 12], 500, lambda r: c(r)["real_swap"] >= 1 and c(r)["thinned"] >= 2)
    print("single")
    cases["single"] = search(au, rng, [260], 300, lambda r: c(r)["self_swap"] == 1)
    print("nobox")
    cases["nobox"] = search(au, rng, [], 300, lambda r: True)
    print("alldrop")
    cases["alldrop"] = search(au, rng, [150, 150, 150], 200, lambda r: c(r)["dropped"] == 3)
    print("paste")
    cases["paste"], paste_names, paste_raw = paste_case(refs, au, iou_fn)
    out = {"cfg_keys": np.array(list(CFG)), "cfg_values": np.array([float(v) for v in CFG.values()]), "tags": np.array(list(cases))}
    for tag, (p, bx, r) in cases.items():
        names = np.array(["Car"] * len(bx))
        if tag == "main":
            names[5] = "Van"                                         # a class-0 box with points
        if tag == "paste":
            names = np.array(paste_names, dtype="<U10")
            for k, v in paste_raw.items():
                out["paste_" + k] = v
        out[tag + "_points"], out[tag + "_boxes"], out[tag + "_names"] = p, bx, names
        for k, v in r["draws"].items():
            if k == "sparsify_keep":
                out[tag + "_keep_len"] = np.array([len(x) for x in v], np.int32)
                out[tag + "_keep"] = np.concatenate(v).astype(np.int32) if v else np.zeros(0, np.int32)
            else:
                out[tag + "_" + k] = v
        out[tag + "_ref_points"], out[tag + "_ref_src"], out[tag + "_ref_flag"] = r["ref_points"], r["ref_src"].astype(np.int32), r["ref_flag"]
        out[tag + "_cover"] = np.array([r["cover"][k] for k in ("dropped", "thinned", "selected_not_thinned", "real_swap", "self_swap", "no_face")], np.int32)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
