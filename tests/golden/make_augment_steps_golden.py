#!/usr/bin/env python
"""Generates tests/golden/augment_steps.npz: the REFERENCE's augmentor steps beyond the four of augment.npz
(pcdet/datasets/augmentor/data_augmentor.py and augmentor_utils.py: random_world_translation,
random_world_frustum_dropout, random_local_translation / _rotation / _scaling / _frustum_dropout, next to gt_sampling and
the world flip / rotation / scaling), run step method by step method in config order on synthetic scenes and a synthetic
database, followed by limit_period and prepare_data's class filter and class column, with every draw recorded:
  * the candidate database ids of every scene and their groups (gt_sampling), as make_augment_golden.py records them;
  * np.random.choice / uniform of the world flip, rotation and scaling -> flip, angle (0: off), scale (1: off);
  * np.random.normal of random_world_translation -> translation (B, axes);
  * np.random.uniform of the dropouts and local steps -> world_dropout (B, directions) and, per local sub-step (one per
    axis or direction), a row of one draw per box alive there (NaN-padded to a common width).
Two configs: `newaugs` is the step list of tools/cfgs/kitti_models/pointpillar_newaugs.yaml (with the
NOISE_TRANSLATE_STD that yaml lacks); `reorder` has no gt_sampling, a world dropout in front of the local translation,
a LOCAL_SCALE_RANGE narrower than 1e-3 and a scalar LOCAL_ROT_ANGLE.

The fixture is made at the level of the step methods, with two departures from DataAugmentor.forward, both stated in
DESIGN.md: boxes outside CLASS_NAMES stay through every step (gt_sampling is given an all-true gt_boxes_mask) and are
dropped at the end, and a box that a world dropout removes takes its name with it (the reference drops the box rows but
not gt_names).

The compiled modules are stubbed as in make_augment_golden.py.  Points carry their identity in a fifth feature column
(scene points 0.., database points negative), so that every in-box test and threshold of the run can be traced back to
raw points: a raw point that at ANY sub-step lies within 1e-4 (float64, on the reference's intermediate state) of a box
face the test reads, or of a dropout threshold, is removed and the case is run again until none is left -- the
reference's draws depend on box counts only.  Box centres within 1e-4 of a world-dropout threshold, or final headings
within 1e-4 of +-pi, reject the attempt.  Only inputs, draws and outputs are stored, plus per output row the number of
rotations it went through and a few coverage counts that tests/test_augment_steps.py asserts.

Run with the reference checkout:  python tests/golden/make_augment_steps_golden.py /path/to/reference
"""
import os
import pathlib
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "augment_steps.npz")
sys.path.insert(0, HERE)
import make_augment_golden as mag  # noqa: E402
from reference_loader import q, reference_root  # noqa: E402
from pdanet_amd.config import to_attr  # noqa: E402

CLASSES = ["Car", "Pedestrian", "Cyclist"]
C = 5
EDGE = 1e-4


class State:
    step = None           # the step method running
    direction = None      # the direction of the dropout function running
    last_uniform = None
    bad_ids = set()       # raw points on a knife edge
    bad_box = False
    box_ids = None        # the original index of every box row alive
    nrot = None           # {point id: local rotations it went through}
    hits = None           # per local sub-step: {point id: boxes that moved it}


ST = State()


class Recorder:
    def __init__(self):
        self.orig = (np.random.permutation, np.random.choice, np.random.uniform, np.random.normal)
        self.events = []

    def __enter__(self):
        rec = self
        perm0, choice0, uniform0, normal0 = self.orig

        def permutation(n):
            out = perm0(n)
            rec.events.append(("perm", np.asarray(out, np.int64).copy()))
            return out

        def choice(a, size=None, replace=True, p=None):
            out = choice0(a, size, replace, p)
            rec.events.append(("choice", bool(out)))
            return out

        def uniform(low=0.0, high=1.0, size=None):
            out = uniform0(low, high, size)
            rec.events.append(("uniform", float(out)))
            ST.last_uniform = float(out)
            return out

        def normal(loc=0.0, scale=1.0, size=None):
            out = normal0(loc, scale, size)
            rec.events.append(("normal", float(np.asarray(out).reshape(-1)[0])))
            return out

        np.random.permutation, np.random.choice, np.random.uniform, np.random.normal = permutation, choice, uniform, normal
        return self

    def __exit__(self, *a):
        np.random.permutation, np.random.choice, np.random.uniform, np.random.normal = self.orig


def instrument(au):
    """Wraps augmentor_utils' in-box test and dropout functions: knife edges in float64, masks, box bookkeeping."""
    gpib0 = au.get_points_in_box

    def get_points_in_box(points, gt_box):
        out, mask = gpib0(points, gt_box)
        p, b = points.astype(np.float64), np.asarray(gt_box, np.float64)
        sx, sy, sz = p[:, 0] - b[0], p[:, 1] - b[1], p[:, 2] - b[2]
        c, s = np.cos(-b[6]), np.sin(-b[6])
        lx, ly = sx * c - sy * s, sx * s + sy * c
        near = (np.abs(np.abs(lx) - (b[3] / 2 + 0.1)) < EDGE) | (np.abs(np.abs(ly) - (b[4] / 2 + 0.1)) < EDGE) | \
               (np.abs(np.abs(sz) - b[5] / 2) < EDGE)
        ids = points[:, 4].astype(np.int64)
        if ST.step == "random_local_frustum_dropout":
            i = ST.last_uniform
            top = ST.direction in ("top", "bottom")
            ctr, ext, col = (b[2], b[5], p[:, 2]) if top else (b[1], b[4], p[:, 1])
            thr = (ctr + ext / 2) - i * ext if ST.direction in ("top", "left") else (ctr - ext / 2) + i * ext
            near |= mask & (np.abs(col - thr) < EDGE)
        else:
            sub = ST.hits[-1]
            for q in ids[mask]:
                sub[int(q)] = sub.get(int(q), 0) + 1
            if ST.step == "random_local_rotation":
                for q in ids[mask]:
                    ST.nrot[int(q)] = ST.nrot.get(int(q), 0) + 1
        ST.bad_ids.update(ids[near].tolist())
        return out, mask

    au.get_points_in_box = get_points_in_box

    def wrap_local(name, direction):
        f0 = getattr(au, name)

        def f(gt_boxes, points, *a, **kw):
            ST.direction = direction
            ST.hits.append({})
            return f0(gt_boxes, points, *a, **kw)
        setattr(au, name, f)

    for d in ("top", "bottom", "left", "right"):
        wrap_local("local_frustum_dropout_" + d, d)
    for a in "xyz":
        wrap_local("random_local_translation_along_" + a, None)
    wrap_local("local_rotation", None)
    wrap_local("local_scaling", None)

    def wrap_world(direction):
        f0 = getattr(au, "global_frustum_dropout_" + direction)

        def f(gt_boxes, points, intensity_range):
            col = 2 if direction in ("top", "bottom") else 1
            p = points[:, col]
            gb, pts = f0(gt_boxes, points, intensity_range)
            i = ST.last_uniform
            mx, mn = np.max(p), np.min(p)
            if direction in ("top", "left"):
                thr = mx - i * (mx - mn)
                keep = gt_boxes[:, col] < thr
                thr64 = float(mx) - i * (float(mx) - float(mn))
            else:
                thr = mn + i * (mx - mn)
                keep = gt_boxes[:, col] > thr
                thr64 = float(mn) + i * (float(mx) - float(mn))
            assert keep.sum() == len(gb) and np.array_equal(gt_boxes[keep], gb)
            ST.box_ids = ST.box_ids[keep]
            ST.bad_ids.update(points[np.abs(p.astype(np.float64) - thr64) < EDGE, 4].astype(np.int64).tolist())
            if len(gt_boxes) and np.min(np.abs(gt_boxes[:, col].astype(np.float64) - thr64)) < EDGE:
                ST.bad_box = True
            return gb, pts
        setattr(au, "global_frustum_dropout_" + direction, f)

    for d in ("top", "bottom", "left", "right"):
        wrap_world(d)


# ---- synthetic scenes: a thin background and a cluster of points in every box -----------------------------------------
def make_scene(rng, n_bg, region, zc, names, extra=()):
    """-> points (n, 4) [x, y, z, intensity], boxes (m, 7), names."""
    pts = [np.stack([rng.uniform(region[0], region[2], n_bg), rng.uniform(region[1], region[3], n_bg),
                     rng.uniform(zc - 0.3, zc + 2.5, n_bg)], 1)]
    boxes = []
    for name in names:
        d = np.array(mag.DIMS[name]) * rng.uniform(0.85, 1.15, 3)
        ctr = [rng.uniform(region[0] + 3, region[2] - 3), rng.uniform(region[1] + 3, region[3] - 3), zc + d[2] / 2]
        boxes.append(ctr + list(d) + [rng.uniform(-np.pi + 0.05, np.pi - 0.05)])
    boxes += [list(b) for b in extra]
    for b in boxes:
        n = int(rng.integers(25, 60))
        lx, ly = rng.uniform(-0.6, 0.6, n) * b[3], rng.uniform(-0.6, 0.6, n) * b[4]
        x, y = mag._rot(lx, ly, b[6])
        pts.append(np.stack([x + b[0], y + b[1], b[2] + rng.uniform(-0.6, 0.6, n) * b[5]], 1))
    p = np.concatenate(pts)
    p = p[rng.permutation(len(p))]
    out = np.zeros((len(p), 4), np.float32)
    out[:, :3] = q(p)
    out[:, 3] = q(rng.uniform(0, 1, len(p)))
    return out, np.array(boxes, np.float32).reshape(-1, 7), np.array(list(names) + ["Car"] * len(extra), dtype="<U10")


NEWAUGS = [
    {"NAME": "gt_sampling", "USE_ROAD_PLANE": False, "DB_INFO_PATH": ["dbinfos.pkl"],
     "PREPARE": {"filter_by_min_points": ["Car:5", "Pedestrian:5", "Cyclist:5"], "filter_by_difficulty": [-1]},
     "SAMPLE_GROUPS": ["Car:4", "Pedestrian:3", "Cyclist:3"], "NUM_POINT_FEATURES": C, "DATABASE_WITH_FAKELIDAR": False,
     "REMOVE_EXTRA_WIDTH": [0.0, 0.0, 0.0], "LIMIT_WHOLE_SCENE": False},
    {"NAME": "random_local_rotation", "LOCAL_ROT_ANGLE": [-0.15707963267, 0.15707963267]},
    {"NAME": "random_local_scaling", "LOCAL_SCALE_RANGE": [0.95, 1.05]},
    {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x"]},
    {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
    {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [0.95, 1.05]},
    {"NAME": "random_world_translation", "NOISE_TRANSLATE_STD": 0.2, "ALONG_AXIS_LIST": ["x", "y", "z"]},
    {"NAME": "random_local_translation", "LOCAL_TRANSLATION_RANGE": [0.95, 1.05], "ALONG_AXIS_LIST": ["x", "y", "z"]},
    {"NAME": "random_world_frustum_dropout", "INTENSITY_RANGE": [0, 0.2], "DIRECTION": ["top"]},
    {"NAME": "random_local_frustum_dropout", "INTENSITY_RANGE": [0, 0.2], "DIRECTION": ["top"]}]
REORDER = [
    {"NAME": "random_world_frustum_dropout", "INTENSITY_RANGE": [0.02, 0.15], "DIRECTION": ["left", "bottom"]},
    {"NAME": "random_local_translation", "LOCAL_TRANSLATION_RANGE": [-0.5, 0.5], "ALONG_AXIS_LIST": ["y", "x"]},
    {"NAME": "random_local_scaling", "LOCAL_SCALE_RANGE": [1.0, 1.0005]},
    {"NAME": "random_local_rotation", "LOCAL_ROT_ANGLE": 0.6},
    {"NAME": "random_world_translation", "NOISE_TRANSLATE_STD": 0.3, "ALONG_AXIS_LIST": ["z", "x"]},
    {"NAME": "random_local_frustum_dropout", "INTENSITY_RANGE": [0.05, 0.3], "DIRECTION": ["right", "bottom", "left"]},
    {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["y", "x"]},
    {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [0.9, 1.1]},
    {"NAME": "random_world_frustum_dropout_disabled_placeholder"}]


def newaugs_case(rng):
    region = (20.0, -8.0, 40.0, 8.0)
    infos, bins = mag.make_db(rng, CLASSES, {"Car": 7, "Pedestrian": 6, "Cyclist": 6}, region, -1.4, 4)
    cfg = {"DISABLE_AUG_LIST": ["placeholder"], "AUG_CONFIG_LIST": NEWAUGS}
    high = [30.0 + rng.uniform(-5, 5), rng.uniform(-5, 5), 0.75, 1.9, 0.8, 0.6, 3.1]     # a box near the top of the scene
    scenes = [make_scene(rng, 1500, region, -1.4, ["Car", "Pedestrian", "Van"]),
              make_scene(rng, 1800, region, -1.4, ["Car", "Car", "Cyclist", "Van"], extra=[high]),
              make_scene(rng, 1200, region, -1.4, [])]
    return cfg, infos, bins, scenes


def reorder_case(rng):
    region = (-30.0, -30.0, 30.0, 30.0)
    cfg = {"DISABLE_AUG_LIST": ["random_world_frustum_dropout_disabled_placeholder"], "AUG_CONFIG_LIST": REORDER}
    a = [5.0, 4.0, -0.8, 4.2, 1.8, 1.6, 0.4]
    b = [6.0, 4.5, -0.7, 4.0, 1.7, 1.5, 2.9]                                            # overlaps a
    low = [-10.0, rng.uniform(-20, 0), -1.62, 0.8, 0.7, 0.3, -3.0]                      # near the bottom
    scenes = [make_scene(rng, 2500, region, -1.6, ["Car", "Van", "Pedestrian"], extra=[a, b]),
              make_scene(rng, 2000, region, -1.6, []),
              make_scene(rng, 2200, region, -1.6, ["Cyclist", "Car", "Van", "Pedestrian"], extra=[low])]
    return cfg, {}, {}, scenes


def with_ids(p4, start, sign=1):
    out = np.zeros((len(p4), C), np.float32)
    out[:, :4] = p4
    out[:, 4] = sign * (start + np.arange(len(p4)))
    return out


def run_case(refs, cfg, infos, bins5, scenes5, seed):
    """-> per scene: out points, out boxes (8), draws, coverage.  bins5 / scenes5 carry the id column."""
    DataAugmentor = refs[0]
    import pcdet.utils.common_utils as cu
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "gt_database"))
    with open(os.path.join(tmp, "dbinfos.pkl"), "wb") as f:
        pickle.dump(infos, f)
    for path, p in bins5.items():
        p.tofile(os.path.join(tmp, path))
    aug = DataAugmentor(pathlib.Path(tmp), to_attr(cfg), CLASSES, logger=None)
    steps = [c for c in cfg["AUG_CONFIG_LIST"] if c["NAME"] not in cfg["DISABLE_AUG_LIST"]]
    tried = []
    if steps[0]["NAME"] == "gt_sampling":
        sampler = aug.data_augmentor_queue[0]
        gid, start = {}, 0
        for name in CLASSES:
            for i, info in enumerate(sampler.db_infos[name]):
                gid[id(info)] = start + i
            start += len(sampler.db_infos[name])
        group_of = {name: g for g, name in enumerate(sampler.sample_groups)}
        orig = sampler.sample_with_fixed_number

        def swf(class_name, sample_group):
            out = orig(class_name, sample_group)
            tried.extend((gid[id(i)], group_of[class_name]) for i in out)
            return out
        sampler.sample_with_fixed_number = swf
    np.random.seed(seed)
    res = []
    for pts, bx, names in scenes5:
        tried.clear()
        ST.nrot, ST.hits, ST.box_ids = {}, [], np.arange(len(bx))
        d = {"points": pts.copy(), "gt_boxes": bx.copy(), "gt_names": names.copy()}
        draws = {"world": [], "translation": [], "world_dropout": [], "local_translation": [], "local_rotation": [],
                 "local_scaling": [], "local_dropout": []}
        cover = dict(wdrop_removed_then_local=0, heading_out=0, n_cand=0, n_acc=0)
        all_names = names.copy()
        for c, fn in zip(steps, aug.data_augmentor_queue):
            ST.step = name = c["NAME"]
            n_before = len(d["gt_boxes"])
            with Recorder() as rec:
                if name == "gt_sampling":
                    d["gt_boxes_mask"] = np.ones(len(d["gt_boxes"]), bool)
                d = fn(data_dict=d)
            ev = [e for e in rec.events if e[0] != "perm"]
            if name == "gt_sampling":
                ST.box_ids = np.arange(len(d["gt_boxes"]))
                all_names = d["gt_names"].copy()
                cover["n_cand"], cover["n_acc"] = len(tried), len(d["gt_boxes"]) - n_before
                draws["cand"] = np.array([t[0] for t in tried], np.int32)
                draws["group"] = np.array([t[1] for t in tried], np.int32)
            elif name in ("random_world_flip", "random_world_rotation", "random_world_scaling"):
                draws["world"] += ev
            elif name == "random_world_translation":
                draws["translation"] = [e[1] for e in ev]
            elif name == "random_world_frustum_dropout":
                draws["world_dropout"] += [e[1] for e in ev]
                if len(d["gt_boxes"]) < n_before:
                    cover["wdrop_removed_then_local"] = -1      # set to 1 by the next local step
            else:
                n_sub = len(c.get("ALONG_AXIS_LIST", c.get("DIRECTION", [0])))
                if name == "random_local_scaling" and c["LOCAL_SCALE_RANGE"][1] - c["LOCAL_SCALE_RANGE"][0] < 1e-3:
                    assert not ev
                    continue
                rows = np.array([e[1] for e in ev], np.float64).reshape(n_sub, -1)
                assert rows.shape[1] == len(d["gt_boxes"])
                draws[{"random_local_frustum_dropout": "local_dropout"}.get(name, name[7:])] = rows
                if cover["wdrop_removed_then_local"] == -1 and len(d["gt_boxes"]):
                    cover["wdrop_removed_then_local"] = 1
                if name == "random_local_rotation" and len(d["gt_boxes"]):
                    cover["heading_out"] = int((np.abs(d["gt_boxes"][:, 6]) > np.pi).sum())
        cover["wdrop_removed_then_local"] = max(cover["wdrop_removed_then_local"], 0)
        gb = d["gt_boxes"]
        gb[:, 6] = cu.limit_period(gb[:, 6], offset=0.5, period=2 * np.pi)
        nm = all_names[ST.box_ids]
        assert len(nm) == len(gb)
        keep = np.array([n in CLASSES for n in nm], bool)
        cls = np.array([CLASSES.index(n) + 1 for n in nm[keep]], np.float32)
        out_boxes = np.concatenate([gb[keep], cls.reshape(-1, 1)], 1).astype(np.float32)
        if len(gb) and np.min(np.pi - np.abs(gb[:, 6].astype(np.float64))) < EDGE:
            ST.bad_box = True
        fx, fy, ang, scl = mag.parse_transform_draws(draws["world"], cfg_only_enabled(cfg))
        ids = d["points"][:, 4].astype(np.int64)
        wrot = int(np.float32(ang) != 0)
        moved_twice = sum(1 for sub in ST.hits for v in sub.values() if v >= 2)
        n_own = len(bx)
        res.append(dict(points=d["points"].astype(np.float32), boxes=out_boxes, draws=draws, flip=(fx, fy), angle=ang, scale=scl,
                        nrot_points=np.array([ST.nrot.get(int(q), 0) + wrot for q in ids], np.int8),
                        nrot_boxes=np.full(len(out_boxes), wrot, np.int8), cover=cover, moved_twice=moved_twice,
                        all_names=all_names, n_own=n_own))
    return res


def cfg_only_enabled(cfg):
    return {"AUG_CONFIG_LIST": [c for c in cfg["AUG_CONFIG_LIST"] if c["NAME"] not in cfg["DISABLE_AUG_LIST"]]}


def build_case(refs, maker, seed0, iou_fn, need):
    for attempt in range(300):
        rng = np.random.default_rng(seed0 + attempt)
        cfg, infos, bins, scenes = maker(rng)
        if infos:
            all_boxes = [i["box3d_lidar"][:7] for name in infos for i in infos[name]] + [b for s in scenes for b in s[1]]
            if not mag._robust_pairs(all_boxes, iou_fn):
                continue
            dbb = np.array([i["box3d_lidar"][:7] for name in infos for i in infos[name]])
            scenes = [(p[~mag._near_face(p, dbb, [0.0, 0.0, 0.0])], bx, nm) for p, bx, nm in scenes]
        removed = set()
        ok = False
        for it in range(30):
            # identities: scene points count up over the batch, database points count down from -1 in path order
            scenes5, at = [], 0
            for p, bx, nm in scenes:
                s5 = with_ids(p, at)
                at += len(p)
                scenes5.append((s5[~np.isin(s5[:, 4].astype(np.int64), list(removed))], bx, nm))
            bins5, at = {}, 1
            for path in sorted(bins):
                b5 = with_ids(bins[path], at, -1)
                at += len(bins[path])
                bins5[path] = b5[~np.isin(b5[:, 4].astype(np.int64), list(removed))]
            ST.bad_ids, ST.bad_box = set(), False
            res = run_case(refs, cfg, infos, bins5, scenes5, 1000 + attempt)
            if ST.bad_box:
                break
            if not ST.bad_ids:
                ok = True
                break
            removed |= ST.bad_ids
        if not ok or not need(res, scenes5):
            continue
        return cfg, infos, bins5, scenes5, res, 1000 + attempt, len(removed)
    raise RuntimeError("no knife-edge-free case found")


def pad_rows(rows_per_scene, n_sub):
    width = max([r.shape[1] for r in rows_per_scene if r is not None and r.size] + [1])
    out = np.full((len(rows_per_scene), n_sub, width), np.nan)
    for b, r in enumerate(rows_per_scene):
        if r is not None and r.size:
            out[b, :, :r.shape[1]] = r
    return out


def main():
    refs = mag.import_reference(reference_root())
    import oracle
    import pcdet.datasets.augmentor.augmentor_utils as au
    instrument(au)

    def iou_fn(a, b):
        a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
        ans = np.zeros((a.shape[0], b.shape[0]), np.float32)
        oracle.boxes_overlap_bev_gpu(a, b, ans)
        return ans

    def need_newaugs(res, scenes5):
        r = res
        return (any(x["cover"]["n_cand"] > x["cover"]["n_acc"] > 0 for x in r) and any(x["cover"]["wdrop_removed_then_local"] for x in r)
                and any(x["cover"]["heading_out"] for x in r) and any(x["angle"] != 0 for x in r) and any(x["flip"][0] for x in r)
                and any(x["moved_twice"] for x in r))

    def need_reorder(res, scenes5):
        r = res
        return (any(x["cover"]["wdrop_removed_then_local"] for x in r) and any(x["cover"]["heading_out"] for x in r)
                and any(x["moved_twice"] for x in r) and any(len(x["boxes"]) == 0 for x in r)
                and any(x["flip"][0] for x in r) and any(x["flip"][1] for x in r))

    data, report = {}, []
    for tag, maker, seed0, need in (("newaugs", newaugs_case, 100, need_newaugs), ("reorder", reorder_case, 400, need_reorder)):
        cfg, infos, bins5, scenes5, res, seed, n_removed = build_case(refs, maker, seed0, iou_fn, need)
        B = len(scenes5)
        enabled = cfg_only_enabled(cfg)["AUG_CONFIG_LIST"]
        by_name = {c["NAME"]: c for c in enabled}
        data[tag + "_class_names"] = np.array(CLASSES)
        data[tag + "_points_raw"] = np.concatenate([s[0] for s in scenes5])
        data[tag + "_offsets"] = np.concatenate([[0], np.cumsum([len(s[0]) for s in scenes5])]).astype(np.int64)
        data[tag + "_boxes_raw"] = np.concatenate([s[1] for s in scenes5]).reshape(-1, 7)
        data[tag + "_box_offsets"] = np.concatenate([[0], np.cumsum([len(s[1]) for s in scenes5])]).astype(np.int64)
        data[tag + "_names_raw"] = np.concatenate([s[2] for s in scenes5]).astype("<U10")
        data[tag + "_aug_cfg"] = np.array(pickle.dumps(cfg, protocol=4))
        data[tag + "_dbinfos"] = np.array(pickle.dumps(infos, protocol=4))
        data[tag + "_db_paths"] = np.array(sorted(bins5))
        data[tag + "_db_points"] = np.concatenate([bins5[p] for p in sorted(bins5)]) if bins5 else np.zeros((0, C), np.float32)
        data[tag + "_db_point_offsets"] = np.concatenate([[0], np.cumsum([len(bins5[p]) for p in sorted(bins5)])]).astype(np.int64)
        cand = [r["draws"].get("cand", np.zeros(0, np.int32)) for r in res]
        data[tag + "_cand"] = np.concatenate(cand).astype(np.int32)
        data[tag + "_cand_group"] = np.concatenate([r["draws"].get("group", np.zeros(0, np.int32)) for r in res]).astype(np.int32)
        data[tag + "_cand_offsets"] = np.concatenate([[0], np.cumsum([len(x) for x in cand])]).astype(np.int64)
        data[tag + "_flip"] = np.array([r["flip"] for r in res], np.int32)
        data[tag + "_angle"] = np.array([r["angle"] for r in res], np.float64)
        data[tag + "_scale"] = np.array([r["scale"] for r in res], np.float32)
        data[tag + "_translation"] = np.array([r["draws"]["translation"] for r in res], np.float64).reshape(B, -1)
        data[tag + "_world_dropout"] = np.array([r["draws"]["world_dropout"] for r in res], np.float64).reshape(B, -1)
        for key, step, sub_key in (("local_translation", "random_local_translation", "ALONG_AXIS_LIST"),
                                   ("local_rotation", "random_local_rotation", None), ("local_scaling", "random_local_scaling", None),
                                   ("local_dropout", "random_local_frustum_dropout", "DIRECTION")):
            rows = [r["draws"][key] if len(r["draws"][key]) else None for r in res]
            if step in by_name and any(x is not None for x in rows):
                data[tag + "_" + key] = pad_rows(rows, len(by_name[step][sub_key]) if sub_key else 1)
        data[tag + "_ref_points"] = np.concatenate([r["points"] for r in res]).astype(np.float32)
        data[tag + "_ref_offsets"] = np.concatenate([[0], np.cumsum([len(r["points"]) for r in res])]).astype(np.int64)
        data[tag + "_ref_boxes"] = np.concatenate([r["boxes"] for r in res]).astype(np.float32).reshape(-1, 8)
        data[tag + "_ref_box_offsets"] = np.concatenate([[0], np.cumsum([len(r["boxes"]) for r in res])]).astype(np.int64)
        data[tag + "_ref_nrot_points"] = np.concatenate([r["nrot_points"] for r in res]).astype(np.int8)
        data[tag + "_ref_nrot_boxes"] = np.concatenate([r["nrot_boxes"] for r in res]).astype(np.int8)
        data[tag + "_cover_moved_twice"] = np.array([r["moved_twice"] for r in res], np.int32)
        data[tag + "_cover_wdrop_then_local"] = np.array([r["cover"]["wdrop_removed_then_local"] for r in res], np.int32)
        data[tag + "_cover_heading_out"] = np.array([r["cover"]["heading_out"] for r in res], np.int32)
        data[tag + "_cover_accepted"] = np.array([r["cover"]["n_acc"] for r in res], np.int32)
        report.append("%s: seed %d, %d knife-edge points removed, raw points %s, raw boxes %s, candidates %s, accepted %s, out points "
                      "%s, out boxes %s, moved twice %s, heading out %s, wdrop then local %s" % (
                          tag, seed, n_removed, [len(s[0]) for s in scenes5], [len(s[1]) for s in scenes5], [len(x) for x in cand],
                          [r["cover"]["n_acc"] for r in res], [len(r["points"]) for r in res], [len(r["boxes"]) for r in res],
                          [r["moved_twice"] for r in res], [r["cover"]["heading_out"] for r in res],
                          [r["cover"]["wdrop_removed_then_local"] for r in res]))
    np.savez_compressed(OUT, **data)
    for r in report:
        print(r)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
