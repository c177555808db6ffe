"""The training-time augmentor on the device (pdanet_amd.data_augmentor, csrc/augment.hip) against the reference's
DataAugmentor recorded in tests/golden/augment.npz (tests/golden/make_augment_golden.py): the sampler bookkeeping, the
database readers and the configuration on the host; on the GPU the augmented scenes, the batch DataProcessor makes of
them, the invariants of the default plan at ONCE size, the no-host-read path and a KITTI training iteration."""
import ctypes
import importlib.util
import os
import pickle

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "augment.npz")
TAGS = ("once", "kitti")
i64 = ctypes.c_int64


def _golden():
    return dict(np.load(GOLDEN))


def _maker():
    spec = importlib.util.spec_from_file_location("make_augment_golden", os.path.join(HERE, "golden", "make_augment_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _rows(g, key, off_key):
    off = g[off_key]
    return [g[key][off[b]:off[b + 1]] for b in range(len(off) - 1)]


def _case(g, tag):
    """-> class names, aug cfg, dbinfos, {path: points}, scenes (points, boxes, names)."""
    names = [str(x) for x in g[tag + "_class_names"]]
    cfg = pickle.loads(g[tag + "_aug_cfg"].item())
    infos = pickle.loads(g[tag + "_dbinfos"].item())
    paths = [str(p) for p in g[tag + "_db_paths"]]
    pts = _rows(g, tag + "_db_points", tag + "_db_point_offsets")
    bins = dict(zip(paths, pts))
    P = _rows(g, tag + "_points_raw", tag + "_offsets")
    Bx = _rows(g, tag + "_boxes_raw", tag + "_box_offsets")
    off = g[tag + "_box_offsets"]
    N = [g[tag + "_names_raw"][off[b]:off[b + 1]] for b in range(len(off) - 1)]
    return names, cfg, infos, bins, list(zip(P, Bx, N))


def _write_db(root, infos, bins):
    os.makedirs(os.path.join(root, "gt_database"), exist_ok=True)
    with open(os.path.join(root, "dbinfos.pkl"), "wb") as f:
        pickle.dump(infos, f)
    for path, p in bins.items():
        p.tofile(os.path.join(root, path))


def _augmentor(g, tag, tmp_path, device="cuda"):
    from pdanet_amd import data_augmentor as da
    names, cfg, infos, bins, scenes = _case(g, tag)
    _write_db(str(tmp_path), infos, bins)
    db = da.GtDatabase.from_dbinfos(str(tmp_path), cfg["AUG_CONFIG_LIST"][0], names, device=device)
    return da.DataAugmentor(cfg, names, db), names, scenes


def _plan(g, tag):
    B = len(g[tag + "_offsets"]) - 1
    return dict(cand=_rows(g, tag + "_cand", tag + "_cand_offsets"), cand_group=_rows(g, tag + "_cand_group", tag + "_cand_offsets"),
                flip_x=g[tag + "_flip"][:, 0], flip_y=g[tag + "_flip"][:, 1], angle=g[tag + "_angle"], scale=g[tag + "_scale"][:B])


def _road(g, tag):
    if tag + "_road_planes" not in g:
        return None, None
    calib = _maker().Calib(g[tag + "_calib_v2c"], g[tag + "_calib_r0"])
    planes = list(g[tag + "_road_planes"])
    return planes, [calib] * len(planes)


# ---- CPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_sampler_bookkeeping_reproduces_the_candidates(tag, tmp_path):
    from pdanet_amd import data_augmentor as da
    g = _golden()
    aug, names, scenes = _augmentor(g, tag, tmp_path, device="cpu")
    perms = iter(_rows(g, tag + "_perms", tag + "_perm_offsets"))
    used = []

    def permutation(n):
        p = next(perms)
        assert len(p) == n
        used.append(n)
        return p

    cand, grp = aug.sample_candidates([da.class_ids(s[2], names) for s in scenes], permutation)
    exp_c = _rows(g, tag + "_cand", tag + "_cand_offsets")
    exp_g = _rows(g, tag + "_cand_group", tag + "_cand_offsets")
    for b in range(len(scenes)):
        assert cand[b].tolist() == exp_c[b].tolist(), b
        assert grp[b].tolist() == exp_g[b].tolist(), b
    assert len(used) == len(g[tag + "_perm_offsets"]) - 1 and len(used) >= 1        # the pointers wrapped


def test_fixture_covers_the_cases():
    g = _golden()
    names, cfg, infos, bins, scenes = _case(g, "once")
    assert any(len(s[1]) == 0 for s in scenes)                                          # a scene with no box
    assert any((s[2] == "Van").any() for s in scenes)                                   # a name outside CLASS_NAMES
    assert (g["once_angle"] == 0).any() and (g["once_angle"] != 0).any()
    assert (g["once_scale"] == 1).any() and g["once_flip"].any(0).all()
    assert any(cfg["AUG_CONFIG_LIST"][0]["REMOVE_EXTRA_WIDTH"])
    assert (np.sum(scenes[2][2] == "Car") >= 5)                                         # LIMIT_WHOLE_SCENE drives Car to <= 0
    cand = _rows(g, "once_cand", "once_cand_offsets")
    out_boxes = np.diff(g["once_ref_box_offsets"])
    kept = [int((s[2] != "Van").sum()) for s in scenes]
    assert any(o < k + len(c) for o, k, c in zip(out_boxes, kept, cand))                # rejected candidates
    assert "kitti_road_planes" in g


def test_from_dbinfos_equals_from_arrays(tmp_path):
    from pdanet_amd import data_augmentor as da
    rng = np.random.default_rng(3)
    infos, bins, boxes, points = {}, {}, {"Car": [], "Cyclist": []}, {"Car": [], "Cyclist": []}
    for name in ("Car", "Cyclist", "Van"):
        infos[name] = []
        for i in range(6):
            n = int(rng.integers(1, 12))
            p = rng.normal(size=(n, 4)).astype(np.float32)
            path = "gt_database/%s_%d.bin" % (name, i)
            bins[path] = p
            box = rng.normal(size=7)
            diff = int(rng.integers(-1, 2))
            infos[name].append({"name": name, "path": path, "box3d_lidar": box, "num_points_in_gt": n, "difficulty": diff})
            if name != "Van" and n >= 5 and diff != -1:
                boxes[name].append(box)
                points[name].append(p)
    _write_db(str(tmp_path), infos, bins)
    cfg = {"DB_INFO_PATH": ["dbinfos.pkl"], "NUM_POINT_FEATURES": 4,
           "PREPARE": {"filter_by_min_points": ["Car:5", "Cyclist:5"], "filter_by_difficulty": [-1]}}
    a = da.GtDatabase.from_dbinfos(str(tmp_path), cfg, ["Car", "Cyclist"], device="cpu")
    b = da.GtDatabase.from_arrays(["Car", "Cyclist"], {k: np.array(v).reshape(-1, 7) for k, v in boxes.items()}, points, device="cpu")
    for key in ("points", "offsets", "boxes", "centre", "classes"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert a.count == b.count and a.count["Car"] == len(boxes["Car"]) and a.n_obj == len(boxes["Car"]) + len(boxes["Cyclist"])
    assert b.centre.dtype == torch.float64 and b.boxes.dtype == torch.float32
    # the shared-memory form: one array and global_data_offset
    allp = np.concatenate([bins[i["path"]] for name in ("Car", "Cyclist") for i in infos[name]])
    at = 0
    for name in ("Car", "Cyclist"):
        for i in infos[name]:
            i["global_data_offset"] = (at, at + len(bins[i["path"]]))
            at += len(bins[i["path"]])
    with open(os.path.join(str(tmp_path), "dbinfos.pkl"), "wb") as f:
        pickle.dump(infos, f)
    np.save(os.path.join(str(tmp_path), "db_data.npy"), allp)
    c = da.GtDatabase.from_dbinfos(str(tmp_path), dict(cfg, USE_SHARED_MEMORY=True, DB_DATA_PATH=["db_data.npy"]),
                                   ["Car", "Cyclist"], device="cpu")
    assert torch.equal(c.points, a.points) and torch.equal(c.offsets, a.offsets)


@pytest.mark.parametrize("yaml_name", ["once_pda_ssd.yaml", "kitti_pda_ssd.yaml"])
def test_reads_the_repo_yamls(yaml_name):
    from pdanet_amd import config, data_augmentor as da
    cfg = config.load_yaml(yaml_name)
    names = list(cfg["CLASS_NAMES"])
    db = da.GtDatabase.from_arrays(names, {n: np.zeros((3, 7)) for n in names},
                                   {n: [np.zeros((2, 4), np.float32)] * 3 for n in names}, device="cpu")
    aug = da.from_config(cfg, db)
    groups = [(gr.name, gr.num) for gr in aug.groups]
    if yaml_name.startswith("once"):
        assert groups == [("Car", 14), ("Bus", 5), ("Truck", 5), ("Pedestrian", 5), ("Cyclist", 13)]
        assert aug.flip_axes == ["x", "y"] and aug.rot_prob == 0.5 and aug.scale_range == [0.9, 1.1] and not aug.use_road_plane
    else:
        assert groups == [("Car", 20), ("Pedestrian", 15), ("Cyclist", 15)]
        assert aug.flip_axes == ["x"] and aug.rot_prob == 1.0 and aug.scale_range == [0.95, 1.05] and aug.use_road_plane
    assert aug.limit_whole_scene
    # DISABLE_AUG_LIST
    block = dict(cfg["DATA_CONFIG"]["DATA_AUGMENTOR"])
    block["DISABLE_AUG_LIST"] = ["gt_sampling", "random_world_rotation"]
    aug = da.DataAugmentor(block, names, None)
    assert aug.groups == [] and aug.rot_range is None and aug.scale_range is not None
    plan = aug.make_plan([np.zeros(0, np.int32)] * 3, np.random.default_rng(0))
    assert "cand" not in plan and (plan["angle"] == 0).all()


def test_refuses_what_it_cannot_run():
    from pdanet_amd import data_augmentor as da
    for step in ("random_world_translation", "random_local_rotation", "random_image_flip"):
        with pytest.raises(NotImplementedError):
            da.DataAugmentor({"AUG_CONFIG_LIST": [{"NAME": step}], "DISABLE_AUG_LIST": []}, ["Car"])
    with pytest.raises(NotImplementedError):
        da.GtDatabase.from_arrays(["Car"], {"Car": np.zeros((1, 9))}, {"Car": [np.zeros((1, 4), np.float32)]}, device="cpu")
    with pytest.raises(ValueError):
        da.DataAugmentor({"AUG_CONFIG_LIST": [{"NAME": "gt_sampling"}], "DISABLE_AUG_LIST": []}, ["Car"])
    aug = da.DataAugmentor({"AUG_CONFIG_LIST": [{"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x"]}],
                            "DISABLE_AUG_LIST": []}, ["Car"])
    with pytest.raises(NotImplementedError):
        aug([np.zeros((4, 4), np.float32)], [np.zeros((1, 9), np.float32)], [np.ones(1, np.int32)])
    assert da.class_ids(["Car", "Van", "Cyclist"], ["Car", "Pedestrian", "Cyclist"]).tolist() == [1, 0, 3]


@pytest.fixture(scope="module")
def lib():
    from pdanet_amd import build, _lib
    build.build()
    return _lib.load()


def test_argument_validation_without_gpu(lib):
    rew = (ctypes.c_float * 3)(0, 0, 0)
    assert lib.pda_augment_workspace_bytes(2, i64(1000), 40) > 0
    assert lib.pda_augment_workspace_bytes(0, i64(1000), 40) >= 0
    assert lib.pda_augment_workspace_bytes(-1, i64(1000), 40) == -1
    assert lib.pda_augment_workspace_bytes(2, i64(0), 40) == -1
    assert lib.pda_augment_workspace_bytes(2, i64(1000), 257) == -1

    def aug(batch=2, c=4, n_cap=10, k=4, n_total=0, m_total=0, paste_cap=0, out_cap=0, box_cap=0):
        return lib.pda_augment(None, None, i64(n_total), batch, c, i64(n_cap), None, None, i64(m_total), None, None, i64(0), None,
                               None, None, 0, None, None, None, k, None, None, None, rew, i64(paste_cap), None, i64(out_cap),
                               None, None, i64(box_cap), None, None, None, None)

    assert aug(batch=0) == 0                                                            # no scene
    assert aug(c=2) == 1 and b"bad size" in lib.pda_last_error()
    assert aug(k=300) == 1 and b"bad size" in lib.pda_last_error()
    assert aug(n_cap=0) == 1 and b"bad size" in lib.pda_last_error()
    assert aug(paste_cap=-1) == 1 and b"bad size" in lib.pda_last_error()
    assert aug(out_cap=-1) == 1 and b"bad size" in lib.pda_last_error()
    assert aug() == 1 and b"null" in lib.pda_last_error()                               # sizes fine, no buffers


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _unpack(pt, bt, info):
    pts, offs, _ = pt
    bx, boffs = bt
    o, bo = offs.cpu().numpy(), boffs.cpu().numpy()
    P, Bx = pts.cpu().numpy(), bx.cpu().numpy()
    return [P[o[b]:o[b + 1]] for b in range(len(o) - 1)], [Bx[bo[b]:bo[b + 1]] for b in range(len(bo) - 1)], info.cpu().numpy()


def _ulps(a, b):
    """|a - b| in float32 steps of the row's largest magnitude: the rotation matmul's rounding is relative to its
    operands, not to a result that cancels towards 0."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    scale = np.maximum(np.abs(a), np.abs(b)).max(axis=-1, keepdims=True)
    return np.abs(a.astype(np.float64) - b) / np.spacing(scale + np.float32(1e-30))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_explicit_plan_gives_the_reference_scenes(tag, tmp_path):
    from pdanet_amd import data_augmentor as da
    g = _golden()
    aug, names, scenes = _augmentor(g, tag, tmp_path)
    planes, calib = _road(g, tag)
    pt, bt, info = aug([s[0] for s in scenes], [s[1] for s in scenes], [da.class_ids(s[2], names) for s in scenes],
                       plan=_plan(g, tag), road_planes=planes, calib=calib)
    P, Bx, info = _unpack(pt, bt, info)
    refP = _rows(g, tag + "_ref_points", tag + "_ref_offsets")
    refB = _rows(g, tag + "_ref_boxes", tag + "_ref_box_offsets")
    for b in range(len(scenes)):
        assert P[b].shape == refP[b].shape and Bx[b].shape == refB[b].shape, b
        assert info[b, 0] == len(refP[b]) and info[b, 1] == len(refB[b]) and info[b, 3] == 0
        assert np.array_equal(Bx[b][:, 7], refB[b][:, 7])                               # box order and class column
        assert np.array_equal(P[b][:, 3:], refP[b][:, 3:])                              # point order (the features)
        assert np.array_equal(Bx[b][:, 3:6], refB[b][:, 3:6])                           # dims: products only
        rot = g[tag + "_angle"][b] != 0
        if not rot and tag == "once":
            assert np.array_equal(P[b], refP[b]) and np.array_equal(Bx[b], refB[b]), b  # bit-exact without the matmul
        else:
            assert _ulps(P[b][:, :3], refP[b][:, :3]).max() <= 4, b
            assert _ulps(Bx[b][:, :7], refB[b][:, :7]).max() <= 4, b
    n_acc = [len(refB[b]) - int((scenes[b][2] != "Van").sum()) if tag == "once" else
             len(refB[b]) - int(np.isin(scenes[b][2], names).sum()) for b in range(len(scenes))]
    assert info[:, 2].tolist() == n_acc


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_augmentor_then_processor_gives_the_reference_batch(tag, tmp_path):
    from pdanet_amd import data_augmentor as da, data_processor as dpm
    g = _golden()
    aug, names, scenes = _augmentor(g, tag, tmp_path)
    planes, calib = _road(g, tag)
    pt, bt, info = aug([s[0] for s in scenes], [s[1] for s in scenes], [da.class_ids(s[2], names) for s in scenes],
                       plan=_plan(g, tag), road_planes=planes, calib=calib)
    k = int(g["num_points"])
    cfg = [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
           {"NAME": "sample_points", "NUM_POINTS": {"train": k, "test": k}},
           {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": True, "test": False}}]
    dp = dpm.DataProcessor(cfg, g[tag + "_range"], True, 4)
    draws = {key: _rows(g, "%s_dp_%s" % (tag, key), "%s_dp_%s_offsets" % (tag, key)) for key in ("pick", "perm1", "perm2")}
    bd = dp(pt, bt, draws=draws)
    ref_p, ref_b = g[tag + "_ref_batch_points"], g[tag + "_ref_batch_gt_boxes"]
    out_p, out_b = bd["points"].cpu().numpy(), bd["gt_boxes"].cpu().numpy()
    assert out_p.shape == ref_p.shape and out_b.shape == ref_b.shape
    assert np.array_equal(out_p[:, [0, 4]], ref_p[:, [0, 4]]) and np.array_equal(out_b[..., 7], ref_b[..., 7])
    assert _ulps(out_p[:, 1:4], ref_p[:, 1:4]).max() <= 4 and _ulps(out_b[..., :7], ref_b[..., :7]).max() <= 4


def _once_size(rng, n_scene=2, n_points=100000, n_db=300):
    from pdanet_amd import data_augmentor as da
    names = ["Car", "Bus", "Truck", "Pedestrian", "Cyclist"]
    dims = {"Car": (4.2, 1.8, 1.6), "Bus": (10.0, 2.8, 3.2), "Truck": (7.0, 2.5, 2.8), "Pedestrian": (0.7, 0.7, 1.7),
            "Cyclist": (1.8, 0.7, 1.5)}
    boxes, points = {}, {}
    for n in names:
        m = n_db // len(names)
        d = np.array(dims[n]) * rng.uniform(0.9, 1.1, (m, 3))
        ctr = np.stack([rng.uniform(-60, 60, m), rng.uniform(-60, 60, m), -1.6 + d[:, 2] / 2], 1)
        boxes[n] = np.concatenate([ctr, d, rng.uniform(-np.pi, np.pi, (m, 1))], 1)
        points[n] = [np.concatenate([rng.uniform(-0.4, 0.4, (k, 3)) * d[i], rng.uniform(0, 1, (k, 1))], 1).astype(np.float32)
                     for i, k in enumerate(rng.integers(5, 200, m))]
    db = da.GtDatabase.from_arrays(names, boxes, points)
    scenes, sboxes, scls = [], [], []
    for b in range(n_scene):
        p = np.concatenate([rng.uniform(-70, 70, (n_points, 2)), rng.uniform(-2, 2, (n_points, 1)), rng.uniform(0, 1, (n_points, 1))], 1)
        scenes.append(p.astype(np.float32))
        m = 12
        d = np.array([dims["Car"]] * m) * rng.uniform(0.9, 1.1, (m, 3))
        ctr = np.stack([rng.uniform(-60, 60, m), rng.uniform(-60, 60, m), -1.6 + d[:, 2] / 2], 1)
        sboxes.append(np.concatenate([ctr, d, rng.uniform(-np.pi, np.pi, (m, 1))], 1).astype(np.float32))
        scls.append(rng.integers(0, 6, m).astype(np.int32))
    cfg = {"DISABLE_AUG_LIST": [], "AUG_CONFIG_LIST": [
        {"NAME": "gt_sampling", "USE_ROAD_PLANE": False, "DB_INFO_PATH": [], "PREPARE": {},
         "SAMPLE_GROUPS": ["Car:14", "Bus:5", "Truck:5", "Pedestrian:5", "Cyclist:13"], "NUM_POINT_FEATURES": 4,
         "REMOVE_EXTRA_WIDTH": [0.1, 0.1, 0.1], "LIMIT_WHOLE_SCENE": True},
        {"NAME": "random_world_flip", "ENABLE_PROB": 0.5, "ALONG_AXIS_LIST": ["x", "y"]},
        {"NAME": "random_world_rotation", "ENABLE_PROB": 1.0, "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
        {"NAME": "random_world_scaling", "ENABLE_PROB": 1.0, "WORLD_SCALE_RANGE": [0.9, 1.1]}]}
    return da.DataAugmentor(cfg, names, db), db, scenes, sboxes, scls


@pytest.mark.gpu
def test_default_plan_invariants_at_once_size():
    from pdanet_amd import _lib  # noqa: F401
    from pdanet_amd.pointnet2_batch_cuda import _call
    rng = np.random.default_rng(5)
    aug, db, scenes, sboxes, scls = _once_size(rng)
    torch.manual_seed(3)
    plan = aug.make_plan(scls)
    pt, bt, info = aug(scenes, sboxes, scls, plan=plan)
    P, Bx, info = _unpack(pt, bt, info)
    for b in range(len(scenes)):
        fx, fy, a, s = int(plan["flip_x"][b]), int(plan["flip_y"][b]), np.float32(plan["angle"][b]), np.float32(plan["scale"][b])
        n_acc = int(info[b, 2])
        keep_cls = scls[b] != 0
        assert info[b, 1] == keep_cls.sum() + n_acc and info[b, 3] == 0
        assert np.array_equal(Bx[b][:keep_cls.sum(), 7], scls[b][keep_cls].astype(np.float32))
        acc = Bx[b][keep_cls.sum():]
        assert ((acc[:, 6] >= -np.pi) & (acc[:, 6] < np.pi)).all() and ((Bx[b][:, 6] >= np.float32(-np.pi)) & (Bx[b][:, 6] < np.float32(np.pi))).all()

        def undo(xyz):
            xyz = xyz.astype(np.float64) / s
            c, sn = np.cos(a), np.sin(a)
            x, y = xyz[:, 0] * c + xyz[:, 1] * sn, -xyz[:, 0] * sn + xyz[:, 1] * c      # the rotation [x, y] R, inverted
            if fy:
                x = -x
            if fx:
                y = -y
            return np.stack([x, y, xyz[:, 2]], 1)
        # the accepted boxes in the scene's own frame: the database boxes, overlapping neither each other nor the scene's
        raw_acc = np.concatenate([undo(acc[:, :3]), acc[:, 3:6] / s], 1)
        ids = [i for i in plan["cand"][b]]
        dbb = db.host_boxes[ids]
        matched = [int(np.argmin(np.abs(dbb[:, :3] - r[:3]).sum(1))) for r in raw_acc]
        assert len(set(matched)) == n_acc and np.abs(dbb[matched, :3] - raw_acc[:, :3]).max() < 1e-3
        acc_raw = np.ascontiguousarray(dbb[matched])
        allb = torch.from_numpy(np.concatenate([sboxes[b], acc_raw])).cuda()
        ov = torch.zeros((len(acc_raw), len(allb)), device="cuda")
        _call("pda_boxes_overlap_bev", ov, torch.from_numpy(acc_raw).cuda().data_ptr(), allb.data_ptr(), ov.data_ptr(), len(acc_raw), len(allb))
        ov = ov.cpu().numpy()
        ov[np.arange(n_acc), len(sboxes[b]) + np.arange(n_acc)] = 0
        assert (ov == 0).all()
        # n_out = pasted + kept; the kept points are the original points outside the enlarged accepted boxes, in order
        n_paste = int(db.sizes[np.array(ids)[matched]].sum())
        kept = undo(P[b][n_paste:, :3])
        raw = scenes[b]
        inside = np.zeros(len(raw), bool)
        for bx in acc_raw:
            cz, h = bx[2], bx[6]
            lx = (raw[:, 0] - bx[0]) * np.cos(-h) - (raw[:, 1] - bx[1]) * np.sin(-h)
            ly = (raw[:, 0] - bx[0]) * np.sin(-h) + (raw[:, 1] - bx[1]) * np.cos(-h)
            inside |= (np.abs(raw[:, 2] - cz) <= (bx[5] + 0.1) / 2) & (np.abs(lx) < (bx[3] + 0.1) / 2 + 1e-2) & (np.abs(ly) < (bx[4] + 0.1) / 2 + 1e-2)
        assert info[b, 0] == n_paste + len(kept)
        assert abs(len(kept) - int((~inside).sum())) <= 2
        if len(kept) == int((~inside).sum()):
            assert np.abs(kept - raw[~inside][:, :3]).max() < 1e-3                     # the inverse transform
            assert np.array_equal(P[b][n_paste:, 3], raw[~inside][:, 3])


@pytest.mark.gpu
def test_no_host_read_with_device_inputs():
    rng = np.random.default_rng(8)
    aug, db, scenes, sboxes, scls = _once_size(rng, n_points=20000, n_db=100)
    packed = torch.from_numpy(np.concatenate(scenes)).cuda()
    offs = torch.tensor([0, len(scenes[0]), len(scenes[0]) + len(scenes[1])], dtype=torch.int64, device="cuda")
    bx = torch.from_numpy(np.concatenate(sboxes)).cuda()
    boffs = torch.tensor([0, len(sboxes[0]), len(sboxes[0]) + len(sboxes[1])], dtype=torch.int64, device="cuda")
    torch.manual_seed(4)
    ref = aug((packed, offs, 20000), (bx, boffs), scls)                                   # loads the kernels
    torch.cuda.synchronize()
    torch.manual_seed(4)
    aug2 = _once_size(np.random.default_rng(8), n_points=20000, n_db=100)[0]
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = aug2((packed, offs, 20000), (bx, boffs), scls, check=False)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.equal(out[0][1], ref[0][1]) and torch.equal(out[1][1], ref[1][1]) and torch.equal(out[2], ref[2])
    n = int(ref[0][1][-1])
    assert torch.equal(out[0][0][:n], ref[0][0][:n])


@pytest.mark.gpu
def test_kitti_training_iteration_on_augmented_scenes():
    from pdanet_amd import data_augmentor as da, data_processor as dpm, detector
    from pdanet_amd.pointnet2_batch_cuda import _call
    mk = _maker()
    rng = np.random.default_rng(9)
    names = ["Car", "Pedestrian", "Cyclist"]
    dims = {"Car": (3.9, 1.6, 1.5), "Pedestrian": (0.8, 0.6, 1.7), "Cyclist": (1.8, 0.6, 1.7)}
    boxes, points = {}, {}
    for n in names:
        m = 20
        d = np.array(dims[n]) * rng.uniform(0.9, 1.1, (m, 3))
        ctr = np.stack([rng.uniform(8, 60, m), rng.uniform(-30, 30, m), -1.7 + d[:, 2] / 2], 1)
        boxes[n] = np.concatenate([ctr, d, rng.uniform(-np.pi, np.pi, (m, 1))], 1)
        points[n] = [np.concatenate([rng.uniform(-0.45, 0.45, (200, 3)) * d[i], rng.uniform(0, 1, (200, 1))], 1).astype(np.float32)
                     for i in range(m)]
    db = da.GtDatabase.from_arrays(names, boxes, points)
    torch.manual_seed(7)
    model, cfg = detector.build_detector("kitti_pda_ssd.yaml")
    model = model.cuda().train()
    aug = da.from_config(cfg, db)
    dp = dpm.from_config(cfg, training=True)
    scenes = [np.concatenate([rng.uniform([2, -38, -2.5, 0], [68, 38, 0.5, 1], (n, 4))]).astype(np.float32) for n in (30000, 18000)]
    sb = [np.array([[20.0, 5.0, -0.9, 3.9, 1.6, 1.5, 0.3]], np.float32), np.zeros((0, 7), np.float32)]
    calib = mk.kitti_calib()
    pt, bt, info = aug(scenes, sb, [np.array([1], np.int32), np.zeros(0, np.int32)],
                       road_planes=[np.array([0.0, -1.0, 0.0, 1.6])] * 2, calib=[calib] * 2)
    assert (info[:, 2] > 0).all().item()
    bd = dp(pt, bt, max_gt=64, seed=5)
    ret, tb, _ = model(bd)
    assert torch.isfinite(ret["loss"])
    ret["loss"].backward()
    # foreground: processed points inside the pasted boxes of the batch
    gt = bd["gt_boxes"]
    pts = bd["points"][:, 1:4].view(2, -1, 3).contiguous()
    idx = torch.full((2, pts.shape[1]), -1, dtype=torch.int32, device="cuda")
    _call("pda_points_in_boxes", gt, gt[..., :7].contiguous().data_ptr(), pts.data_ptr(), idx.data_ptr(), 2, gt.shape[1], pts.shape[1])
    n_fix = [1, 0]
    for b in range(2):
        pasted = idx[b] >= n_fix[b]
        assert int(pasted.sum()) > 50
