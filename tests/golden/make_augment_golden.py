#!/usr/bin/env python
"""Generates tests/golden/augment.npz: the REFERENCE's training-time augmentor
(pcdet/datasets/augmentor/data_augmentor.py DataAugmentor with database_sampler.py DataBaseSampler: gt_sampling ->
random_world_flip -> random_world_rotation -> random_world_scaling -> limit_period), followed by prepare_data's class
filter and class column (pcdet/datasets/dataset.py), run on synthetic scenes and a synthetic database (a dbinfos pickle
and per-object .bin files written to a temporary directory), with every draw it makes recorded:
  * np.random.permutation in sample_with_fixed_number (a class pointer wrapped) -> `perms`, in call order;
  * np.random.choice([False, True], ...) and np.random.uniform -> per scene flip_x, flip_y, angle (0: rotation not
    enabled), scale (1: scaling not enabled);
  * the candidate database ids of every scene, in the order the sampler tried them, and their class groups.
The augmented scenes then go through the reference DataProcessor (mask_points_and_boxes_outside_range -> sample_points
-> shuffle_points) and collate_batch with their draws recorded as make_input_golden.py records them (end-to-end case).

The compiled modules are stubbed (through reference_loader.py).  points_in_boxes_cpu is a numpy statement of
roiaware_pool3d.cpp:121-170 (the CPU test, margin 1e-2) and boxes_bev_iou_cpu is the repository's C oracle of the BEV overlap (oracle/, the
iou3d_nms_kernel.cu statement): like the other fixtures, this pins the reference's Python composition, not its C++
arithmetic.  Inputs are kept away from knife edges so that either arithmetic decides alike: box pairs overlap clearly or
stay 1e-3 apart, scene points stay 1e-4 or more from every enlarged database box face, final coordinates stay 1e-4 or
more from the range planes and the 40 m sphere, final headings 1e-4 or more from +-pi.  Only inputs and outputs are
stored.

Run with the reference checkout:  python tests/golden/make_augment_golden.py /path/to/reference
"""
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from reference_loader import cpu_torch, load, points_in_boxes_cpu_np, q as _q, reference_root  # noqa: E402
import oracle  # noqa: E402
from pdanet_amd.config import AttrDict as AD, to_attr as _ad  # noqa: E402

OUT = os.path.join(HERE, "augment.npz")
K = 2048
ONCE_CLASSES = ["Car", "Bus", "Truck", "Pedestrian", "Cyclist"]
KITTI_CLASSES = ["Car", "Pedestrian", "Cyclist"]
ONCE_RANGE = [-75.2, -75.2, -5.0, 75.2, 75.2, 3.0]
KITTI_RANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
DIMS = {"Car": (4.2, 1.8, 1.6), "Bus": (10.0, 2.8, 3.2), "Truck": (7.0, 2.5, 2.8), "Pedestrian": (0.7, 0.7, 1.7),
        "Cyclist": (1.8, 0.7, 1.5), "Van": (5.0, 2.0, 2.0)}


class Calib:
    """A KITTI-style calibration (lidar -> rect: V2C then R0) with the two methods put_boxes_on_road_planes calls."""

    def __init__(self, v2c, r0):
        self.V2C, self.R0 = np.asarray(v2c, np.float64), np.asarray(r0, np.float64)

    def lidar_to_rect(self, pts):
        hom = np.hstack([pts, np.ones((pts.shape[0], 1), np.float32)])
        return np.dot(hom, np.dot(self.V2C.T, self.R0.T))

    def rect_to_lidar(self, pts):
        r0 = np.eye(4)
        r0[:3, :3] = self.R0
        v2c = np.eye(4)
        v2c[:3, :4] = self.V2C
        hom = np.hstack([pts, np.ones((pts.shape[0], 1))])
        return np.dot(hom, np.linalg.inv(np.dot(r0, v2c)).T)[:, :3]


def kitti_calib():
    v2c = [[0.0, -1.0, 0.0, 0.02], [0.0, 0.0, -1.0, -0.08], [1.0, 0.0, 0.0, -0.27]]
    a = 0.01
    r0 = [[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]]
    return Calib(v2c, r0)


def import_reference(root):
    """-> (DataAugmentor, DataBaseSampler, DataProcessor, DatasetTemplate) of the reference, loaded as pcdet.*"""
    import torch
    cpu_torch()
    oracle.build()

    def boxes_bev_iou_cpu(a, b):
        a = np.ascontiguousarray(np.asarray(a, np.float32)[:, :7])
        b = np.ascontiguousarray(np.asarray(b, np.float32)[:, :7])
        ans = np.zeros((a.shape[0], b.shape[0]), np.float32)
        if a.shape[0] and b.shape[0]:
            oracle.boxes_iou_bev_gpu(a, b, ans)
        return ans

    def points_in_boxes_cpu(points, boxes):
        pts = points.numpy() if isinstance(points, torch.Tensor) else points
        bx = boxes.numpy() if isinstance(boxes, torch.Tensor) else boxes
        return torch.from_numpy(points_in_boxes_cpu_np(pts, bx))

    stubs = {"ops.roiaware_pool3d.roiaware_pool3d_utils": {"points_in_boxes_cpu": points_in_boxes_cpu},
             "ops.iou3d_nms.iou3d_nms_utils": {"boxes_bev_iou_cpu": boxes_bev_iou_cpu},
             "datasets.processor.point_feature_encoder": {"PointFeatureEncoder": None}}
    da, dbs, dp, ds = load(root, "pcdet", ["datasets.augmentor.data_augmentor", "datasets.augmentor.database_sampler",
                                           "datasets.processor.data_processor", "datasets.dataset"], stubs=stubs, real_paths=True)
    return da.DataAugmentor, dbs.DataBaseSampler, dp.DataProcessor, ds.DatasetTemplate


# ---- synthetic database and scenes --------------------------------------------------------------------------------------
def _rot(x, y, h):
    c, s = np.cos(h), np.sin(h)
    return x * c - y * s, x * s + y * c


def make_db(rng, classes, counts, region, zc, c):
    """dbinfos {name: [info]}: boxes in `region` (x0, y0, x1, y1), object points relative to the centre."""
    infos, bins = {}, {}
    for name in classes + ["Van"]:
        lst = []
        for i in range(counts.get(name, 3)):
            d = np.array(DIMS[name]) * rng.uniform(0.85, 1.15, 3)
            ctr = [rng.uniform(region[0], region[2]), rng.uniform(region[1], region[3]), zc + d[2] / 2]
            h = rng.uniform(-np.pi + 0.05, np.pi - 0.05)
            box = np.array(ctr + list(d) + [h], np.float64)
            n = int(rng.integers(3, 30))
            lx = rng.uniform(-0.45, 0.45, n) * d[0]
            ly = rng.uniform(-0.45, 0.45, n) * d[1]
            x, y = _rot(lx, ly, h)
            p = np.zeros((n, c), np.float32)
            p[:, 0], p[:, 1] = _q(x), _q(y)
            p[:, 2] = _q(rng.uniform(-0.45, 0.45, n) * d[2])
            p[:, 3:] = _q(rng.uniform(0, 1, (n, c - 3)))
            path = "gt_database/%s_%d.bin" % (name, i)
            bins[path] = p
            lst.append({"name": name, "path": path, "box3d_lidar": box, "num_points_in_gt": n,
                        "difficulty": int(rng.integers(-1, 3)), "gt_idx": i})
        infos[name] = lst
    return infos, bins


def make_scene(rng, n, region, zc, c, names, box_region):
    p = np.zeros((n, c), np.float32)
    p[:, 0] = _q(rng.uniform(region[0], region[2], n))
    p[:, 1] = _q(rng.uniform(region[1], region[3], n))
    p[:, 2] = _q(rng.uniform(zc - 0.3, zc + 2.5, n))
    p[:, 3:] = _q(rng.uniform(0, 1, (n, c - 3)))
    boxes = []
    for name in names:
        d = np.array(DIMS[name]) * rng.uniform(0.85, 1.15, 3)
        ctr = [rng.uniform(box_region[0], box_region[2]), rng.uniform(box_region[1], box_region[3]), zc + d[2] / 2]
        boxes.append(ctr + list(d) + [rng.uniform(-np.pi + 0.05, np.pi - 0.05)])
    return p, np.array(boxes, np.float32).reshape(-1, 7), np.array(names, dtype="<U10")


def _robust_pairs(all_boxes, iou_fn):
    """every pair either overlaps when both shrink by 1e-3 or stays apart when both grow by 1e-3."""
    b = np.asarray(all_boxes, np.float32)
    g, s = b.copy(), b.copy()
    g[:, 3:5] += 2e-3
    s[:, 3:5] -= 2e-3
    og, os_ = iou_fn(g, g) > 0, iou_fn(s, s) > 0
    np.fill_diagonal(og, False)
    np.fill_diagonal(os_, False)
    return np.array_equal(og, os_)


def _near_face(points, boxes, ew):
    """points within 1e-4 of a face of any box enlarged by ew (in the box frame)."""
    bad = np.zeros(points.shape[0], bool)
    for b in np.asarray(boxes, np.float64):
        sx, sy = points[:, 0] - b[0], points[:, 1] - b[1]
        lx, ly = _rot(sx, sy, -b[6])
        hx, hy, hz = (b[3] + ew[0]) / 2, (b[4] + ew[1]) / 2, (b[5] + ew[2]) / 2
        for v, h in ((lx, hx + 1e-2), (ly, hy + 1e-2), (points[:, 2] - b[2], hz)):
            bad |= np.abs(np.abs(v) - h) < 1e-4
    return bad


# ---- recording ---------------------------------------------------------------------------------------------------------
class AugRecorder:
    def __init__(self):
        self.orig = (np.random.permutation, np.random.choice, np.random.uniform)
        self.events = []

    def __enter__(self):
        rec = self
        perm0, choice0, uniform0 = self.orig

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
            return out

        np.random.permutation, np.random.choice, np.random.uniform = permutation, choice, uniform
        return self

    def __exit__(self, *a):
        np.random.permutation, np.random.choice, np.random.uniform = self.orig


def parse_transform_draws(events, aug_cfg):
    """the choice / uniform events of one scene -> flip_x, flip_y, angle, scale."""
    ev = [e for e in events if e[0] != "perm"]
    fx = fy = 0
    angle, scale = 0.0, 1.0
    at = 0
    for cfg in aug_cfg["AUG_CONFIG_LIST"]:
        if cfg["NAME"] == "random_world_flip":
            for ax in cfg["ALONG_AXIS_LIST"]:
                on = ev[at][1]
                at += 1
                if ax == "x":
                    fx = int(on)
                else:
                    fy = int(on)
        elif cfg["NAME"] == "random_world_rotation":
            on = ev[at][1]
            at += 1
            if on:
                angle = ev[at][1]
                at += 1
        elif cfg["NAME"] == "random_world_scaling":
            r = cfg["WORLD_SCALE_RANGE"]
            if r[1] - r[0] >= 1e-3:
                on = ev[at][1]
                at += 1
                if on:
                    scale = ev[at][1]
                    at += 1
    assert at == len(ev), (at, ev)
    return fx, fy, angle, np.float32(scale)


def run_case(refs, tag, classes, aug_cfg, infos, bins, scenes, road, seed, pr):
    DataAugmentor, DataBaseSampler, DataProcessor, DatasetTemplate = refs
    tmp = tempfile.mkdtemp()
    import pathlib
    os.makedirs(os.path.join(tmp, "gt_database"))
    with open(os.path.join(tmp, "dbinfos.pkl"), "wb") as f:
        pickle.dump(infos, f)
    for path, p in bins.items():
        p.tofile(os.path.join(tmp, path))
    aug = DataAugmentor(pathlib.Path(tmp), _ad(aug_cfg), classes, logger=None)
    sampler = aug.data_augmentor_queue[0]
    gid = {}
    start = 0
    for name in classes:
        for i, info in enumerate(sampler.db_infos[name]):
            gid[id(info)] = start + i
        start += len(sampler.db_infos[name])
    group_of = {name: g for g, name in enumerate(sampler.sample_groups)}
    tried = []
    orig = sampler.sample_with_fixed_number

    def swf(class_name, sample_group):
        out = orig(class_name, sample_group)
        tried.extend((gid[id(i)], group_of[class_name]) for i in out)
        return out

    sampler.sample_with_fixed_number = swf
    np.random.seed(seed)
    fake = types.SimpleNamespace(training=True, class_names=classes, data_augmentor=aug,
                                 point_feature_encoder=types.SimpleNamespace(forward=lambda d: d),
                                 data_processor=types.SimpleNamespace(forward=lambda data_dict: data_dict))
    outs, draws = [], []
    for b, (pts, bx, names) in enumerate(scenes):
        tried.clear()
        d = {"points": pts.copy(), "gt_boxes": bx.copy(), "gt_names": names.copy()}
        if road is not None:
            d["road_plane"], d["calib"] = road[0][b], road[1]
        with AugRecorder() as rec:
            d = DatasetTemplate.prepare_data(fake, d)
        fx, fy, ang, scl = parse_transform_draws(rec.events, aug_cfg)
        draws.append(dict(cand=np.array([t[0] for t in tried], np.int32), group=np.array([t[1] for t in tried], np.int32),
                          perms=[e[1] for e in rec.events if e[0] == "perm"], flip_x=fx, flip_y=fy, angle=ang, scale=scl))
        outs.append(d)
    return tmp, outs, draws


def run_processor(refs, outs, pr, c, seed):
    sys.path.insert(0, HERE)
    import make_input_golden as mig
    DataProcessor, DatasetTemplate = refs[2], refs[3]
    cfg = [AD(NAME="mask_points_and_boxes_outside_range", REMOVE_OUTSIDE_BOXES=True),
           AD(NAME="sample_points", NUM_POINTS=AD(train=K, test=K)),
           AD(NAME="shuffle_points", SHUFFLE_ENABLED=AD(train=True, test=False))]
    dp = DataProcessor(cfg, np.array(pr, np.float32), True, c)
    np.random.seed(seed)
    rec = mig.Recorder()
    res, draws = [], {"pick": [], "perm1": [], "perm2": []}
    with rec:
        for d in outs:
            rec.reset()
            res.append(dp.forward({"points": d["points"].copy(), "gt_boxes": d["gt_boxes"].copy()}))
            draws["pick"].append(rec.pick)
            draws["perm1"].append(rec.perm1)
            draws["perm2"].append(rec.perm2)
    return DatasetTemplate.collate_batch(res), draws


def once_case(rng):
    c = 4
    classes = ONCE_CLASSES
    region = (-30.0, -30.0, 30.0, 30.0)
    infos, bins = make_db(rng, classes, {"Car": 9, "Bus": 4, "Truck": 4, "Pedestrian": 7, "Cyclist": 6}, region, -1.6, c)
    aug_cfg = {"DISABLE_AUG_LIST": ["placeholder"], "AUG_CONFIG_LIST": [
        {"NAME": "gt_sampling", "USE_ROAD_PLANE": False, "DB_INFO_PATH": ["dbinfos.pkl"],
         "PREPARE": {"filter_by_min_points": ["Car:5", "Bus:5", "Truck:5", "Pedestrian:5", "Cyclist:5"]},
         "SAMPLE_GROUPS": ["Car:5", "Bus:2", "Truck:2", "Pedestrian:3", "Cyclist:3"], "NUM_POINT_FEATURES": c,
         "REMOVE_EXTRA_WIDTH": [0.2, 0.1, 0.05], "LIMIT_WHOLE_SCENE": True},
        {"NAME": "random_world_flip", "ENABLE_PROB": 0.5, "ALONG_AXIS_LIST": ["x", "y"]},
        {"NAME": "random_world_rotation", "ENABLE_PROB": 0.5, "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
        {"NAME": "random_world_scaling", "ENABLE_PROB": 0.5, "WORLD_SCALE_RANGE": [0.9, 1.1]}]}
    names = [["Car", "Pedestrian", "Van", "Cyclist"], [], ["Car"] * 6 + ["Truck"], ["Bus", "Van", "Pedestrian"],
             ["Cyclist", "Car"]]
    scenes = [make_scene(rng, int(rng.integers(2500, 3500)), (-40, -40, 40, 40), -1.6, c, nm, region) for nm in names]
    return c, classes, aug_cfg, infos, bins, scenes, None, ONCE_RANGE


def kitti_case(rng):
    c = 4
    classes = KITTI_CLASSES
    region = (20.0, -8.0, 40.0, 8.0)
    infos, bins = make_db(rng, classes, {"Car": 7, "Pedestrian": 6, "Cyclist": 6}, region, -1.4, c)
    aug_cfg = {"DISABLE_AUG_LIST": ["placeholder"], "AUG_CONFIG_LIST": [
        {"NAME": "gt_sampling", "USE_ROAD_PLANE": True, "DB_INFO_PATH": ["dbinfos.pkl"],
         "PREPARE": {"filter_by_min_points": ["Car:5", "Pedestrian:5", "Cyclist:5"], "filter_by_difficulty": [-1]},
         "SAMPLE_GROUPS": ["Car:4", "Pedestrian:3", "Cyclist:3"], "NUM_POINT_FEATURES": c, "DATABASE_WITH_FAKELIDAR": False,
         "REMOVE_EXTRA_WIDTH": [0.0, 0.0, 0.0], "LIMIT_WHOLE_SCENE": True},
        {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x"]},
        {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
        {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [0.95, 1.05]}]}
    names = [["Car", "Pedestrian"], ["Car", "Car", "Cyclist", "Van"], ["Pedestrian"]]
    scenes = [make_scene(rng, int(rng.integers(1500, 2200)), (20, -8, 40, 8), -1.4, c, nm, region) for nm in names]
    planes = [np.array([0.01 * b, -1.0, 0.02, 1.55 + 0.03 * b]) for b in range(len(scenes))]
    return c, classes, aug_cfg, infos, bins, scenes, (planes, kitti_calib()), KITTI_RANGE


def _final_ok(outs, pr):
    for d in outs:
        p, bx = d["points"], d["gt_boxes"]
        for a in (0, 1):
            if np.min(np.abs(p[:, a:a + 1] - np.float32([pr[a], pr[3 + a]]))) < 1e-4:
                return False
        if np.min(np.abs(np.linalg.norm(p[:, :3].astype(np.float64), axis=1) - 40.0)) < 1e-4:
            return False
        if len(bx) and np.min(np.pi - np.abs(bx[:, 6].astype(np.float64))) < 1e-4:
            return False
    return True


def build_case(refs, maker, seed0, iou_fn, need):
    for attempt in range(200):
        rng = np.random.default_rng(seed0 + attempt)
        c, classes, aug_cfg, infos, bins, scenes, road, pr = maker(rng)
        all_boxes = [i["box3d_lidar"][:7] for name in infos for i in infos[name]] + [b for s in scenes for b in s[1]]
        if not _robust_pairs(all_boxes, iou_fn):
            continue
        ew = aug_cfg["AUG_CONFIG_LIST"][0]["REMOVE_EXTRA_WIDTH"]
        dbb = np.array([i["box3d_lidar"][:7] for name in infos for i in infos[name]])
        if road is not None:      # the road-plane shift moves the boxes in z: test the faces at the shifted heights too
            shifted = []
            for b in range(len(scenes)):
                a_, b_, c_, d_ = road[0][b]
                cam = road[1].lidar_to_rect(dbb[:, :3].astype(np.float32))
                cam[:, 1] = (-d_ - a_ * cam[:, 0] - c_ * cam[:, 2]) / b_
                h = road[1].rect_to_lidar(cam)[:, 2]
                s = dbb.copy()
                s[:, 2] = h + s[:, 5] / 2
                shifted.append(s)
            face_boxes = [np.concatenate([dbb] + shifted)] * len(scenes)
        else:
            face_boxes = [dbb] * len(scenes)
        scenes = [(p[~_near_face(p, fb, ew)], bx, nm) for (p, bx, nm), fb in zip(scenes, face_boxes)]
        tmp, outs, draws = run_case(refs, None, classes, aug_cfg, infos, bins, scenes, road, 1000 + attempt, pr)
        if not _final_ok(outs, pr):
            continue
        if not need(draws, outs, scenes):
            continue
        return c, classes, aug_cfg, infos, bins, scenes, road, pr, tmp, outs, draws, 1000 + attempt
    raise RuntimeError("no knife-edge-free case found")


def main():
    refs = import_reference(reference_root())

    def iou_fn(a, b):
        a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
        ans = np.zeros((a.shape[0], b.shape[0]), np.float32)
        oracle.boxes_overlap_bev_gpu(a, b, ans)
        return ans

    def need_once(draws, outs, scenes):
        rot_off = any(d["angle"] == 0.0 for d in draws)
        scl_off = any(d["scale"] == 1.0 for d in draws)
        rot_on = any(d["angle"] != 0.0 for d in draws)
        flips = any(d["flip_x"] for d in draws) and any(d["flip_y"] for d in draws)
        wrap = sum(len(d["perms"]) for d in draws) >= 1
        rejected = any(len(o["gt_boxes"]) < int((sc[2] != "Van").sum()) + len(d["cand"]) for o, d, sc in zip(outs, draws, scenes))
        return rot_off and scl_off and rot_on and flips and wrap and rejected

    def need_kitti(draws, outs, scenes):
        return any(d["flip_x"] for d in draws)

    data, report = {}, []
    for tag, maker, seed0, need in (("once", once_case, 100, need_once), ("kitti", kitti_case, 300, need_kitti)):
        c, classes, aug_cfg, infos, bins, scenes, road, pr, tmp, outs, draws, seed = build_case(refs, maker, seed0, iou_fn, need)
        B = len(scenes)
        batch, pdraws = run_processor(refs, outs, pr, c, seed + 7)
        # inputs
        data[tag + "_class_names"] = np.array(classes)
        data[tag + "_range"] = np.array(pr, np.float32)
        data[tag + "_points_raw"] = np.concatenate([s[0] for s in scenes])
        data[tag + "_offsets"] = np.concatenate([[0], np.cumsum([len(s[0]) for s in scenes])]).astype(np.int64)
        data[tag + "_boxes_raw"] = np.concatenate([s[1] for s in scenes]).reshape(-1, 7)
        data[tag + "_box_offsets"] = np.concatenate([[0], np.cumsum([len(s[1]) for s in scenes])]).astype(np.int64)
        data[tag + "_names_raw"] = np.concatenate([s[2] for s in scenes]).astype("<U10")
        data[tag + "_aug_cfg"] = np.array(pickle.dumps(aug_cfg, protocol=4))
        data[tag + "_dbinfos"] = np.array(pickle.dumps(infos, protocol=4))
        data[tag + "_db_paths"] = np.array(sorted(bins))
        data[tag + "_db_points"] = np.concatenate([bins[p] for p in sorted(bins)])
        data[tag + "_db_point_offsets"] = np.concatenate([[0], np.cumsum([len(bins[p]) for p in sorted(bins)])]).astype(np.int64)
        if road is not None:
            data[tag + "_road_planes"] = np.stack(road[0])
            data[tag + "_calib_v2c"] = road[1].V2C
            data[tag + "_calib_r0"] = road[1].R0
        # draws
        data[tag + "_cand"] = np.concatenate([d["cand"] for d in draws]).astype(np.int32)
        data[tag + "_cand_group"] = np.concatenate([d["group"] for d in draws]).astype(np.int32)
        data[tag + "_cand_offsets"] = np.concatenate([[0], np.cumsum([len(d["cand"]) for d in draws])]).astype(np.int64)
        perms = [p for d in draws for p in d["perms"]]
        data[tag + "_perms"] = np.concatenate(perms).astype(np.int32) if perms else np.zeros(0, np.int32)
        data[tag + "_perm_offsets"] = np.concatenate([[0], np.cumsum([len(p) for p in perms])]).astype(np.int64)
        data[tag + "_flip"] = np.array([[d["flip_x"], d["flip_y"]] for d in draws], np.int32)
        data[tag + "_angle"] = np.array([d["angle"] for d in draws], np.float64)
        data[tag + "_scale"] = np.array([d["scale"] for d in draws], np.float32)
        # outputs
        data[tag + "_ref_points"] = np.concatenate([o["points"] for o in outs]).astype(np.float32)
        data[tag + "_ref_offsets"] = np.concatenate([[0], np.cumsum([len(o["points"]) for o in outs])]).astype(np.int64)
        data[tag + "_ref_boxes"] = np.concatenate([o["gt_boxes"] for o in outs]).astype(np.float32).reshape(-1, 8)
        data[tag + "_ref_box_offsets"] = np.concatenate([[0], np.cumsum([len(o["gt_boxes"]) for o in outs])]).astype(np.int64)
        for key in ("pick", "perm1", "perm2"):
            data[tag + "_dp_" + key] = np.concatenate(pdraws[key]).astype(np.int32)
            data[tag + "_dp_" + key + "_offsets"] = np.concatenate([[0], np.cumsum([len(x) for x in pdraws[key]])]).astype(np.int64)
        data[tag + "_ref_batch_points"] = batch["points"].astype(np.float32)
        data[tag + "_ref_batch_gt_boxes"] = batch["gt_boxes"].astype(np.float32)
        report.append("%s: seed %d, raw points %s, raw boxes %s, candidates %s, out boxes %s, perms %d, draws %s" % (
            tag, seed, [len(s[0]) for s in scenes], [len(s[1]) for s in scenes], [len(d["cand"]) for d in draws],
            [len(o["gt_boxes"]) for o in outs], len(perms),
            [(d["flip_x"], d["flip_y"], round(d["angle"], 3), float(d["scale"])) for d in draws]))
    data["num_points"] = np.array(K)
    np.savez_compressed(OUT, **data)
    for r in report:
        print(r)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
