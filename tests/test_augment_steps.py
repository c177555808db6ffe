"""The augmentor's ordered step program (pdanet_amd/data_augmentor.py, csrc/augment_steps.hip: pda_augment_paste +
pda_augment_steps) against the reference's step methods recorded in tests/golden/augment_steps.npz
(tests/golden/make_augment_steps_golden.py), and against a float32 numpy restatement of the per-point walk kept here."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "augment_steps.npz")
TAGS = ("newaugs", "reorder")
i64 = ctypes.c_int64
f32 = np.float32
LOCAL_KEYS = ("local_translation", "local_rotation", "local_scaling", "local_dropout")


def _golden():
    return dict(np.load(GOLDEN))


def _rows(g, key, off_key):
    off = g[off_key]
    return [g[key][off[b]:off[b + 1]] for b in range(len(off) - 1)]


def _case(g, tag):
    names = [str(x) for x in g[tag + "_class_names"]]
    cfg = pickle.loads(g[tag + "_aug_cfg"].item())
    infos = pickle.loads(g[tag + "_dbinfos"].item())
    paths = [str(p) for p in g[tag + "_db_paths"]]
    bins = dict(zip(paths, _rows(g, tag + "_db_points", tag + "_db_point_offsets")))
    P = _rows(g, tag + "_points_raw", tag + "_offsets")
    Bx = _rows(g, tag + "_boxes_raw", tag + "_box_offsets")
    off = g[tag + "_box_offsets"]
    N = [g[tag + "_names_raw"][off[b]:off[b + 1]] for b in range(len(off) - 1)]
    return names, cfg, infos, bins, list(zip(P, Bx, N))


def _plan(g, tag):
    B = len(g[tag + "_offsets"]) - 1
    plan = dict(cand=_rows(g, tag + "_cand", tag + "_cand_offsets"), cand_group=_rows(g, tag + "_cand_group", tag + "_cand_offsets"),
                flip_x=g[tag + "_flip"][:, 0], flip_y=g[tag + "_flip"][:, 1], angle=g[tag + "_angle"], scale=g[tag + "_scale"],
                translation=g[tag + "_translation"], world_dropout=g[tag + "_world_dropout"])
    for key in LOCAL_KEYS:
        if tag + "_" + key in g:                       # NaN-padded (B, sub-steps, width): the recorded rows are ragged
            plan[key] = [[r[~np.isnan(r)] for r in g[tag + "_" + key][b]] for b in range(B)]
    return plan


def _augmentor(g, tag, tmp_path, device="cuda"):
    from pdanet_amd import data_augmentor as da
    names, cfg, infos, bins, scenes = _case(g, tag)
    db = None
    if infos:
        os.makedirs(os.path.join(str(tmp_path), "gt_database"), exist_ok=True)
        with open(os.path.join(str(tmp_path), "dbinfos.pkl"), "wb") as f:
            pickle.dump(infos, f)
        for path, p in bins.items():
            p.tofile(os.path.join(str(tmp_path), path))
        db = da.GtDatabase.from_dbinfos(str(tmp_path), cfg["AUG_CONFIG_LIST"][0], names, device=device)
    return da.DataAugmentor(cfg, names, db), names, scenes


# ---- the per-point walk in float32 numpy --------------------------------------------------------------------------------
def _cs(a):
    return f32(np.cos(np.float64(a))), f32(np.sin(np.float64(a)))


def _rot(x, y, c, s):
    return x * c + y * (-s), x * s + y * c


def walk(points, boxes8, ops, scene_draws, box_draws):
    """One scene through the program, every operation a separately rounded float32 one (float64 where the reference's is),
    as csrc/augment_steps.hip states them.  points (n, C) float32, boxes8 (m, 8); ops (n_ops, 2); scene_draws (n_ops);
    box_draws (local ops, D).  -> points out, boxes out (m', 8): limit_period applied, class 0 dropped."""
    P = np.array(points, f32)
    bx = np.array(boxes8, f32)
    pi = f32(3.14159265358979323846)
    local = 0
    for (code, arg), d in zip(np.asarray(ops).tolist(), np.asarray(scene_draws, np.float64).tolist()):
        if code == 0:
            if d != 0:
                P[:, 1], bx[:, 1], bx[:, 6] = -P[:, 1], -bx[:, 1], -bx[:, 6]
        elif code == 1:
            if d != 0:
                P[:, 0], bx[:, 0], bx[:, 6] = -P[:, 0], -bx[:, 0], -(bx[:, 6] + pi)
        elif code == 2:
            a = f32(d)
            if a != 0:
                c, s = _cs(a)
                P[:, 0], P[:, 1] = _rot(P[:, 0].copy(), P[:, 1].copy(), c, s)
                bx[:, 0], bx[:, 1] = _rot(bx[:, 0].copy(), bx[:, 1].copy(), c, s)
                bx[:, 6] = bx[:, 6] + a
        elif code == 3:
            P[:, :3] = P[:, :3] * f32(d)
            bx[:, :6] = bx[:, :6] * f32(d)
        elif code == 4:
            P[:, arg] = (P[:, arg].astype(np.float64) + d).astype(f32)
            bx[:, arg] = (bx[:, arg].astype(np.float64) + d).astype(f32)
        elif code == 5:
            col = 2 if arg < 2 else 1
            if len(P) == 0:
                bx = bx[:0]
                continue
            mx, mn = P[:, col].max(), P[:, col].min()
            span = f32(d) * (mx - mn)
            if arg in (0, 2):
                thr = mx - span
                P, bx = P[P[:, col] < thr], bx[bx[:, col] < thr]
            else:
                thr = mn + span
                P, bx = P[P[:, col] > thr], bx[bx[:, col] > thr]
        else:
            row = box_draws[local]
            local += 1
            for j in range(len(bx)):
                f = f32(row[j])
                cx, cy, cz, dx, dy, dz, h = bx[j, :7]
                ca, sa = _cs(-h)
                sx, sy, sz = P[:, 0] - cx, P[:, 1] - cy, P[:, 2] - cz
                lx, ly = _rot(sx, sy, ca, sa)
                m = (np.abs(sz) <= dz / f32(2)) & (np.abs(lx) <= dx / f32(2) + f32(0.1)) & (np.abs(ly) <= dy / f32(2) + f32(0.1))
                if code == 6:
                    P[m, arg] = P[m, arg] + f
                    bx[j, arg] = bx[j, arg] + f
                elif code == 7:
                    c, s = _cs(f)
                    x, y = _rot(sx[m], sy[m], c, s)
                    P[m, 0], P[m, 1], P[m, 2] = x + cx, y + cy, sz[m] + cz
                    bx[j, 6] = h + f
                elif code == 8:
                    P[m, 0], P[m, 1], P[m, 2] = sx[m] * f + cx, sy[m] * f + cy, sz[m] * f + cz
                    bx[j, 3:6] = bx[j, 3:6] * f
                else:
                    ctr, ext, col = (cz, dz, 2) if arg < 2 else (cy, dy, 1)
                    if arg in (0, 2):
                        hit = P[:, col] >= (ctr + ext / f32(2)) - f * ext
                    else:
                        hit = P[:, col] <= (ctr - ext / f32(2)) + f * ext
                    P = P[~(m & hit)]
    two_pi = f32(6.28318530717958647692)
    bx[:, 6] = bx[:, 6] - np.floor(bx[:, 6] / two_pi + f32(0.5)) * two_pi
    return P, bx[bx[:, 7] != 0]


def _ulps(a, b):
    """|a - b| in float32 steps of the row's largest magnitude (tests/test_augment.py _ulps)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    scale = np.maximum(np.abs(a), np.abs(b)).max(axis=-1, keepdims=True)
    return np.abs(a.astype(np.float64) - b) / np.spacing(scale + f32(1e-30))


def _compare_with_reference(g, tag, b, P, Bx):
    """Every point and every box of scene b against the recorded reference scene."""
    refP = _rows(g, tag + "_ref_points", tag + "_ref_offsets")[b]
    refB = _rows(g, tag + "_ref_boxes", tag + "_ref_box_offsets")[b]
    nrp = _rows(g, tag + "_ref_nrot_points", tag + "_ref_offsets")[b].astype(np.int64)
    nrb = _rows(g, tag + "_ref_nrot_boxes", tag + "_ref_box_offsets")[b].astype(np.int64)
    assert P.shape == refP.shape and Bx.shape == refB.shape, (tag, b, P.shape, refP.shape, Bx.shape, refB.shape)
    assert np.array_equal(Bx[:, 7], refB[:, 7])                                         # box order and class column
    assert np.array_equal(P[:, 3:], refP[:, 3:])                                        # point order (features, identity)
    assert np.array_equal(Bx[:, 3:6], refB[:, 3:6])                                     # dims: products only
    assert np.array_equal(P[nrp == 0], refP[nrp == 0])                                  # bit-exact without a rotation
    assert np.array_equal(Bx[nrb == 0], refB[nrb == 0])
    if (nrp > 0).any():
        u = _ulps(P[nrp > 0, :3], refP[nrp > 0, :3]).max(axis=1)
        print("%s scene %d: %d rotated points, worst %.2f steps per rotation" % (tag, b, (nrp > 0).sum(), (u / nrp[nrp > 0]).max()))
        assert (u <= 4 * nrp[nrp > 0]).all()
    if (nrb > 0).any():
        u = _ulps(Bx[nrb > 0, :7], refB[nrb > 0, :7]).max(axis=1)
        assert (u <= 4 * nrb[nrb > 0]).all()


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_fixture_covers_the_cases():
    g = _golden()
    cfgs = {tag: pickle.loads(g[tag + "_aug_cfg"].item()) for tag in TAGS}
    steps = {tag: {c["NAME"]: c for c in cfgs[tag]["AUG_CONFIG_LIST"] if c["NAME"] not in cfgs[tag]["DISABLE_AUG_LIST"]} for tag in TAGS}
    order = {tag: list(steps[tag]) for tag in TAGS}
    # the pointpillar_newaugs order: local rotation and scaling in front of the world transforms, the rest behind them
    assert order["newaugs"] == ["gt_sampling", "random_local_rotation", "random_local_scaling", "random_world_flip",
                                "random_world_rotation", "random_world_scaling", "random_world_translation",
                                "random_local_translation", "random_world_frustum_dropout", "random_local_frustum_dropout"]
    assert "gt_sampling" not in order["reorder"]
    assert order["reorder"].index("random_world_frustum_dropout") < order["reorder"].index("random_local_translation")
    assert len(steps["newaugs"]["random_world_translation"]["ALONG_AXIS_LIST"]) == 3     # NOISE_TRANSLATE_STD on three axes
    assert steps["newaugs"]["random_world_translation"]["NOISE_TRANSLATE_STD"] > 0
    r = steps["reorder"]["random_local_scaling"]["LOCAL_SCALE_RANGE"]
    assert r[1] - r[0] < 1e-3 and "reorder_local_scaling" not in g                       # a skipped local scaling
    for tag in TAGS:
        assert (g[tag + "_cover_moved_twice"] > 0).any(), tag                            # a point in two boxes that both move it
        assert (g[tag + "_cover_wdrop_then_local"] > 0).any(), tag                       # a world dropout removed a box, a local step after
        assert (g[tag + "_cover_heading_out"] > 0).any(), tag                            # a heading outside [-pi, pi) after local rotation
    n_cand = np.diff(g["newaugs_cand_offsets"])
    acc = g["newaugs_cover_accepted"]
    assert ((acc > 0) & (acc < n_cand)).any()                                            # a rejected candidate
    assert (g["newaugs_ref_points"][:, 4] < 0).any()                                     # pasted points went through the local steps
    assert (np.diff(g["reorder_box_offsets"]) == 0).any()                                # a scene with no box
    # a class-0 box with points inside it (the raw box against the raw points, the in-box test of the local steps)
    found = 0
    for tag in TAGS:
        names, _, _, _, scenes = _case(g, tag)
        for p, bx, nm in scenes:
            for box, n in zip(bx, nm):
                if n in names:
                    continue
                sx, sy, sz = p[:, 0] - box[0], p[:, 1] - box[1], p[:, 2] - box[2]
                lx, ly = _rot(sx, sy, *_cs(-box[6]))
                found += int(((np.abs(sz) <= box[5] / 2) & (np.abs(lx) <= box[3] / 2 + 0.1) & (np.abs(ly) <= box[4] / 2 + 0.1)).sum() > 0)
    assert found
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("tag", TAGS)
def test_constructs_from_the_fixture_configs(tag):
    from pdanet_amd import data_augmentor as da
    g = _golden()
    names, cfg, infos, bins, scenes = _case(g, tag)
    db = None
    if infos:
        boxes = {n: np.stack([i["box3d_lidar"] for i in infos[n]]) for n in names}
        pts = {n: [bins[i["path"]] for i in infos[n]] for n in names}
        db = da.GtDatabase.from_arrays(names, boxes, pts, device="cpu")
    aug = da.DataAugmentor(cfg, names, db)
    assert aug.program is not None and all(0 <= st[0] <= 9 for st in aug.program)
    if tag == "newaugs":
        assert [st[0] for st in aug.program] == [da.OP_LROT, da.OP_LSCALE, da.OP_FLIP_X, da.OP_ROT, da.OP_SCALE, da.OP_TRANS, da.OP_TRANS,
                                                 da.OP_TRANS, da.OP_LTRANS, da.OP_LTRANS, da.OP_LTRANS, da.OP_WDROP, da.OP_LDROP]
    else:                                              # the narrow local scaling is no op; y before x as the yaml lists them
        assert [(st[0], st[1]) for st in aug.program] == [
            (da.OP_WDROP, 2), (da.OP_WDROP, 1), (da.OP_LTRANS, 1), (da.OP_LTRANS, 0), (da.OP_LROT, 0), (da.OP_TRANS, 2), (da.OP_TRANS, 0),
            (da.OP_LDROP, 3), (da.OP_LDROP, 1), (da.OP_LDROP, 2), (da.OP_FLIP_Y, 0), (da.OP_FLIP_X, 0), (da.OP_SCALE, 0)]
    # a list works like the dict; the four first steps alone keep the pda_augment path
    assert da.DataAugmentor([c for c in cfg["AUG_CONFIG_LIST"] if c["NAME"] not in cfg["DISABLE_AUG_LIST"]], names, db).program is not None
    legacy = [c for c in cfg["AUG_CONFIG_LIST"] if c["NAME"] in ("gt_sampling", "random_world_flip", "random_world_rotation", "random_world_scaling")]
    assert da.DataAugmentor(legacy, names, db).program is None


def test_constructs_from_a_yaml_shaped_dict():
    from pdanet_amd import data_augmentor as da
    cfg = {"CLASS_NAMES": ["Car"], "DATA_CONFIG": {"DATA_AUGMENTOR": {
        "DISABLE_AUG_LIST": ["random_local_translation"],
        "AUG_CONFIG_LIST": [{"NAME": "random_local_rotation", "LOCAL_ROT_ANGLE": [-0.15707963267, 0.15707963267]},
                            {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x"]},
                            {"NAME": "random_world_translation", "NOISE_TRANSLATE_STD": 0, "ALONG_AXIS_LIST": ["x", "y", "z"]},
                            {"NAME": "random_local_translation"},
                            {"NAME": "random_world_frustum_dropout", "INTENSITY_RANGE": [0, 0.2], "DIRECTION": ["top"]}]}}}
    aug = da.from_config(cfg)
    # NOISE_TRANSLATE_STD 0 is no op (the reference returns before a draw); a disabled entry is not looked at
    assert [(st[0], st[1]) for st in aug.program] == [(da.OP_LROT, 0), (da.OP_FLIP_X, 0), (da.OP_WDROP, 0)]


def test_missing_parameter_rule():
    from pdanet_amd import data_augmentor as da
    full = {"random_world_translation": {"NOISE_TRANSLATE_STD": 0.2, "ALONG_AXIS_LIST": ["x"]},
            "random_local_translation": {"LOCAL_TRANSLATION_RANGE": [0.9, 1.1], "ALONG_AXIS_LIST": ["x"]},
            "random_local_rotation": {"LOCAL_ROT_ANGLE": 0.1}, "random_local_scaling": {"LOCAL_SCALE_RANGE": [0.9, 1.1]},
            "random_world_frustum_dropout": {"INTENSITY_RANGE": [0, 0.2], "DIRECTION": ["top"]},
            "random_local_frustum_dropout": {"INTENSITY_RANGE": [0, 0.2], "DIRECTION": ["left"]}}
    for step, params in full.items():
        da.DataAugmentor([dict(NAME=step, **params)], ["Car"])
        for key in params:
            entry = dict(NAME=step, **{k: v for k, v in params.items() if k != key})
            with pytest.raises(NotImplementedError) as e:
                da.DataAugmentor([entry], ["Car"])
            assert step in str(e.value) and key in str(e.value)
    for step in ("random_image_flip", "random_local_pyramid_aug"):
        with pytest.raises(NotImplementedError):
            da.DataAugmentor([{"NAME": step}], ["Car"])
    with pytest.raises(NotImplementedError):                                            # a step appears at most once
        da.DataAugmentor([dict(NAME="random_local_rotation", LOCAL_ROT_ANGLE=0.1)] * 2, ["Car"])


def test_make_plan_shapes_and_reproducibility():
    from pdanet_amd import data_augmentor as da
    g = _golden()
    names, cfg, infos, bins, scenes = _case(g, "newaugs")
    boxes = {n: np.stack([i["box3d_lidar"] for i in infos[n]]) for n in names}
    pts = {n: [bins[i["path"]] for i in infos[n]] for n in names}
    cls = [da.class_ids(s[2], names) for s in scenes]

    def plan(seed):
        torch.manual_seed(seed)
        aug = da.DataAugmentor(cfg, names, da.GtDatabase.from_arrays(names, boxes, pts, device="cpu"))
        return aug.make_plan(cls)

    p = plan(11)
    B = len(scenes)
    D = max(len(cls[b]) + len(p["cand"][b]) for b in range(B))
    assert p["translation"].shape == (B, 3) and p["world_dropout"].shape == (B, 1)
    assert p["local_rotation"].shape == (B, D) and p["local_scaling"].shape == (B, D)
    assert p["local_translation"].shape == (B, 3, D) and p["local_dropout"].shape == (B, 1, D)
    assert (np.abs(p["local_rotation"]) <= 0.15707963267).all() and ((p["local_scaling"] >= 0.95) & (p["local_scaling"] <= 1.05)).all()
    assert ((p["world_dropout"] >= 0) & (p["world_dropout"] <= 0.2)).all() and ((p["local_translation"] >= 0.95) & (p["local_translation"] <= 1.05)).all()
    q, r = plan(11), plan(12)
    for key in ("translation", "world_dropout", "angle", "scale") + LOCAL_KEYS:
        assert np.array_equal(p[key], q[key]), key
    assert not np.array_equal(p["local_rotation"], r["local_rotation"])


@pytest.fixture(scope="module")
def lib():
    from pdanet_amd import build, _lib
    build.build()
    return _lib.load()


def test_argument_validation_without_gpu(lib):
    assert lib.pda_abi_version() == 20
    assert lib.pda_augment_steps_workspace_bytes(2, i64(1000), 40, 13) > 0
    assert lib.pda_augment_steps_workspace_bytes(0, i64(1000), 0, 0) >= 0
    assert lib.pda_augment_steps_workspace_bytes(-1, i64(1000), 40, 13) == -1
    assert lib.pda_augment_steps_workspace_bytes(2, i64(0), 40, 13) == -1
    assert lib.pda_augment_steps_workspace_bytes(2, i64(1000), 257, 13) == -1
    assert lib.pda_augment_steps_workspace_bytes(2, i64(1000), 40, 33) == -1
    ops = (ctypes.c_int32 * 4)(7, 0, 5, 0)

    def steps(batch=2, c=5, n_cap=10, n_ops=2, draw_cap=4, slots=4, out_cap=0, box_cap=0, ops=ops):
        return lib.pda_augment_steps(None, None, i64(0), batch, c, i64(n_cap), None, None, i64(0), ops, n_ops, None, None, draw_cap,
                                     slots, None, None, i64(out_cap), None, None, i64(box_cap), None, None, None, None)

    assert steps(batch=0) == 0                                                          # no scene
    assert steps(c=2) == 1 and b"bad size" in lib.pda_last_error()
    assert steps(n_cap=0) == 1 and b"bad size" in lib.pda_last_error()
    assert steps(n_ops=33) == 1 and b"bad size" in lib.pda_last_error()
    assert steps(slots=300) == 1 and b"bad size" in lib.pda_last_error()
    assert steps(draw_cap=-1) == 1 and b"bad size" in lib.pda_last_error()
    assert steps(out_cap=-1) == 1 and b"bad size" in lib.pda_last_error()
    assert steps(ops=(ctypes.c_int32 * 4)(10, 0, 5, 0)) == 1 and b"bad op" in lib.pda_last_error()
    assert steps(ops=(ctypes.c_int32 * 4)(5, 4, 5, 0)) == 1 and b"bad op" in lib.pda_last_error()
    five = (ctypes.c_int32 * 10)(5, 0, 5, 1, 5, 2, 5, 3, 5, 0)
    assert steps(ops=five, n_ops=5) == 1 and b"bad size" in lib.pda_last_error()        # more than four world dropouts
    assert steps() == 1 and b"null" in lib.pda_last_error()                             # sizes fine, no buffers
    rew = (ctypes.c_float * 3)(0, 0, 0)

    def paste(batch=2, c=4, k=4, paste_cap=0):
        return lib.pda_augment_paste(None, None, i64(0), batch, c, i64(10), None, None, i64(0), None, None, i64(0), None, None, None, 0,
                                     None, None, None, k, rew, i64(paste_cap), None, i64(0), None, None, i64(0), None, None, None, None)

    assert paste(batch=0) == 0
    assert paste(k=300) == 1 and b"pda_augment_paste: bad size" in lib.pda_last_error()
    assert paste() == 1 and b"null" in lib.pda_last_error()


def test_float32_walk_gives_the_reference_scenes():
    """The restatement the kernel is held to: on the `reorder` config (no paste, so it starts from the raw scenes) it
    gives the reference's scenes, bit for bit where no rotation is involved."""
    from pdanet_amd import data_augmentor as da
    tag = "reorder"
    g = _golden()
    names, cfg, infos, bins, scenes = _case(g, tag)
    aug = da.DataAugmentor(cfg, names, None)
    plan = _plan(g, tag)
    B = len(scenes)
    ops, scene_draws, box_draws, D = aug._program_draws(plan, B, np.asarray(plan["flip_x"]), np.asarray(plan["flip_y"]),
                                                         np.asarray(plan["angle"], np.float64), np.asarray(plan["scale"], f32))
    for b, (p, bx, nm) in enumerate(scenes):
        b8 = np.concatenate([bx, da.class_ids(nm, names).astype(f32).reshape(-1, 1)], 1)
        P, Bx = walk(p, b8, ops, scene_draws[b], box_draws[b])
        _compare_with_reference(g, tag, b, P, Bx)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _unpack(pt, bt, info):
    pts, offs, _ = pt
    bx, boffs = bt
    o, bo = offs.cpu().numpy(), boffs.cpu().numpy()
    P, Bx = pts.cpu().numpy(), bx.cpu().numpy()
    return [P[o[b]:o[b + 1]] for b in range(len(o) - 1)], [Bx[bo[b]:bo[b + 1]] for b in range(len(bo) - 1)], info.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_recorded_draws_give_the_reference_scenes(tag, tmp_path):
    from pdanet_amd import data_augmentor as da
    g = _golden()
    aug, names, scenes = _augmentor(g, tag, tmp_path)
    pt, bt, info = aug([s[0] for s in scenes], [s[1] for s in scenes], [da.class_ids(s[2], names) for s in scenes], plan=_plan(g, tag))
    P, Bx, info = _unpack(pt, bt, info)
    refP = _rows(g, tag + "_ref_points", tag + "_ref_offsets")
    refB = _rows(g, tag + "_ref_boxes", tag + "_ref_box_offsets")
    for b in range(len(scenes)):
        assert info[b, 0] == len(refP[b]) and info[b, 1] == len(refB[b])
        assert info[b, 3] == (0 if len(refB[b]) else da.STATUS_NO_BOX)                   # a scene left without a box is flagged
        _compare_with_reference(g, tag, b, P[b], Bx[b])
    assert info[:, 2].tolist() == [a if len(refB[b]) else 0 for b, a in enumerate(g[tag + "_cover_accepted"].tolist())]


def _random_scene(rng, n_points, m, c=5, id0=0, extent=30.0):
    dims = np.array([(4.2, 1.8, 1.6), (0.7, 0.7, 1.7), (1.8, 0.7, 1.5), (10.0, 2.8, 3.2)])
    d = dims[rng.integers(0, 4, m)] * rng.uniform(0.9, 1.1, (m, 3))
    ctr = np.stack([rng.uniform(-extent, extent, m), rng.uniform(-extent, extent, m), -1.6 + d[:, 2] / 2], 1)
    bx = np.concatenate([ctr, d, rng.uniform(-np.pi, np.pi, (m, 1))], 1).astype(f32)
    n_in = n_points // 2 if m else 0                         # half the points inside boxes, so that the local steps have work
    k = rng.integers(0, m, n_in)
    loc = rng.uniform(-0.6, 0.6, (n_in, 3)) * bx[k, 3:6]
    c_, s_ = np.cos(bx[k, 6]), np.sin(bx[k, 6])
    inb = np.stack([loc[:, 0] * c_ - loc[:, 1] * s_ + bx[k, 0], loc[:, 0] * s_ + loc[:, 1] * c_ + bx[k, 1], loc[:, 2] + bx[k, 2]], 1)
    bg = np.concatenate([rng.uniform(-extent - 5, extent + 5, (n_points - n_in, 2)), rng.uniform(-2, 2, (n_points - n_in, 1))], 1)
    p = np.zeros((n_points, c), f32)
    p[:, :3] = np.concatenate([inb, bg])[rng.permutation(n_points)]
    p[:, 3] = rng.uniform(0, 1, n_points)
    p[:, 4] = id0 + np.arange(n_points)
    return p, bx


FULL_LIST = [
    {"NAME": "random_local_rotation", "LOCAL_ROT_ANGLE": [-0.3, 0.3]},
    {"NAME": "random_local_scaling", "LOCAL_SCALE_RANGE": [0.9, 1.1]},
    {"NAME": "random_world_frustum_dropout", "INTENSITY_RANGE": [0.02, 0.1], "DIRECTION": ["right", "top"]},
    {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x", "y"], "ENABLE_PROB": 1.0},
    {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
    {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [0.95, 1.05]},
    {"NAME": "random_world_translation", "NOISE_TRANSLATE_STD": 0.2, "ALONG_AXIS_LIST": ["x", "y", "z"]},
    {"NAME": "random_local_translation", "LOCAL_TRANSLATION_RANGE": [-0.4, 0.4], "ALONG_AXIS_LIST": ["x", "y", "z"]},
    {"NAME": "random_local_frustum_dropout", "INTENSITY_RANGE": [0, 0.3], "DIRECTION": ["top", "bottom", "left", "right"]}]


@pytest.mark.gpu
def test_kernel_matches_the_float32_walk_bit_for_bit():
    """100 000 points and 60 boxes (a third of them of class 0), nothing filtered: the kernel's own arithmetic, rotation
    included, where the reference's matmul is loose."""
    from pdanet_amd import data_augmentor as da
    rng = np.random.default_rng(21)
    p, bx = _random_scene(rng, 100000, 60)
    cls = rng.integers(0, 3, 60).astype(np.int32)
    p2, bx2 = _random_scene(rng, 3000, 0)                                                # and a scene without a box
    aug = da.DataAugmentor(FULL_LIST, ["Car", "Pedestrian"], None)
    torch.manual_seed(5)
    classes = [cls, np.zeros(0, np.int32)]
    plan = aug.make_plan(classes)
    pt, bt, info = aug([p, p2], [bx, bx2], classes, plan=plan)
    P, Bx, info = _unpack(pt, bt, info)
    ops, scene_draws, box_draws, D = aug._program_draws(plan, 2, plan["flip_x"], plan["flip_y"], plan["angle"], plan["scale"])
    for b, (pp, bb, cc) in enumerate(((p, bx, cls), (p2, bx2, classes[1]))):
        wP, wB = walk(pp, np.concatenate([bb, cc.astype(f32).reshape(-1, 1)], 1), ops, scene_draws[b], box_draws[b])
        print("scene %d: %d -> %d points (walk %d), %d -> %d boxes (walk %d)" % (b, len(pp), len(P[b]), len(wP), len(bb), len(Bx[b]), len(wB)))
        assert P[b].shape == wP.shape and Bx[b].shape == wB.shape
        assert np.array_equal(P[b], wP) and np.array_equal(Bx[b], wB)
        assert info[b].tolist() == [len(wP), len(wB), 0, 0 if len(wB) and len(wP) else da.STATUS_NO_BOX]
    assert len(P[0]) < 100000 and 0 < len(Bx[0]) < 60 and (P[0][:, :3] != p[np.isin(p[:, 4], P[0][:, 4])][:, :3]).any()


def _small_db(rng, names, n_each=20, c=4, id0=None):
    dims = {"Car": (3.9, 1.6, 1.5), "Pedestrian": (0.8, 0.6, 1.7), "Cyclist": (1.8, 0.6, 1.7)}
    boxes, points = {}, {}
    at = 1
    for n in names:
        d = np.array(dims[n]) * rng.uniform(0.9, 1.1, (n_each, 3))
        ctr = np.stack([rng.uniform(8, 60, n_each), rng.uniform(-30, 30, n_each), -1.7 + d[:, 2] / 2], 1)
        boxes[n] = np.concatenate([ctr, d, rng.uniform(-np.pi, np.pi, (n_each, 1))], 1)
        points[n] = []
        for i in range(n_each):
            q = np.zeros((200, c), f32)
            q[:, :3] = rng.uniform(-0.45, 0.45, (200, 3)) * d[i]
            q[:, 3] = rng.uniform(0, 1, 200)
            if c > 4:
                q[:, 4] = -(at + np.arange(200))
                at += 200
            points[n].append(q)
    return boxes, points


@pytest.mark.gpu
def test_a_config_of_the_four_old_steps_takes_the_parent_path():
    """DataAugmentor with only gt_sampling and the world flip / rotation / scaling has no program and gives the tensors
    pda_augment gives when called directly with the same plan."""
    from pdanet_amd import data_augmentor as da, _lib
    rng = np.random.default_rng(13)
    names = ["Car", "Pedestrian", "Cyclist"]
    boxes, points = _small_db(rng, names)
    db = da.GtDatabase.from_arrays(names, boxes, points)
    cfg = [{"NAME": "gt_sampling", "USE_ROAD_PLANE": False, "DB_INFO_PATH": [], "PREPARE": {}, "SAMPLE_GROUPS": ["Car:6", "Pedestrian:4", "Cyclist:4"],
            "NUM_POINT_FEATURES": 4, "REMOVE_EXTRA_WIDTH": [0.1, 0.1, 0.0], "LIMIT_WHOLE_SCENE": False},
           {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x", "y"]},
           {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
           {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [0.95, 1.05]}]
    aug = da.DataAugmentor(cfg, names, db)
    assert aug.program is None
    scenes = [rng.uniform([2, -38, -2.5, 0], [68, 38, 0.5, 1], (n, 4)).astype(f32) for n in (20000, 12000)]
    sb = [np.array([[20.0, 5.0, -0.9, 3.9, 1.6, 1.5, 0.3], [30.0, -5.0, -0.9, 3.9, 1.6, 1.5, 2.0]], f32), np.zeros((0, 7), f32)]
    cls = [np.array([1, 0], np.int32), np.zeros(0, np.int32)]
    torch.manual_seed(2)
    plan = aug.make_plan(cls)
    pt, bt, info = aug(scenes, sb, cls, plan=plan)
    # pda_augment directly
    lib = _lib.load()
    B, K, C = 2, max(len(r) for r in plan["cand"]), 4
    cand = np.full((B, K), -1, np.int32)
    grp = np.full((B, K), -1, np.int32)
    for b in range(B):
        cand[b, :len(plan["cand"][b])] = plan["cand"][b]
        grp[b, :len(plan["cand"][b])] = plan["cand_group"][b]
    paste = [int(db.sizes[plan["cand"][b]].sum()) for b in range(B)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n_total, m_total, n_cap = sum(len(s) for s in scenes), 2, max(len(s) for s in scenes)
    d_pts, d_off = dev(np.concatenate(scenes)), dev(np.array([0, len(scenes[0]), n_total], np.int64))
    d_bx = dev(np.concatenate([np.concatenate(sb), np.concatenate(cls).astype(f32).reshape(-1, 1)], 1))
    d_boff = dev(np.array([0, 2, 2], np.int64))
    d_cand, d_grp, d_dz = dev(cand), dev(grp), dev(np.zeros((B, K)))
    d_flip = dev(np.stack([plan["flip_x"], plan["flip_y"]], 1).astype(np.int32))
    d_angle, d_scale = dev(np.asarray(plan["angle"], np.float64)), dev(np.asarray(plan["scale"], f32))
    ws = torch.empty(lib.pda_augment_workspace_bytes(B, i64(n_cap), K), dtype=torch.uint8, device="cuda")
    out_cap, box_cap = n_total + sum(paste), m_total + int((cand >= 0).sum())
    out = torch.empty((out_cap, C), device="cuda")
    ob = torch.empty((box_cap, 8), device="cuda")
    oo, obo = torch.empty(B + 1, dtype=torch.int64, device="cuda"), torch.empty(B + 1, dtype=torch.int64, device="cuda")
    inf = torch.empty((B, 4), dtype=torch.int32, device="cuda")
    rew = (ctypes.c_float * 3)(0.1, 0.1, 0.0)
    st = lib.pda_augment(d_pts.data_ptr(), d_off.data_ptr(), i64(n_total), B, C, i64(n_cap), d_bx.data_ptr(), d_boff.data_ptr(), i64(m_total),
                         db.points.data_ptr(), db.offsets.data_ptr(), i64(db.points.shape[0]), db.boxes.data_ptr(), db.centre.data_ptr(),
                         db.classes.data_ptr(), db.n_obj, d_cand.data_ptr(), d_grp.data_ptr(), d_dz.data_ptr(), K, d_flip.data_ptr(),
                         d_angle.data_ptr(), d_scale.data_ptr(), rew, i64(max(paste)), out.data_ptr(), i64(out_cap), oo.data_ptr(),
                         ob.data_ptr(), i64(box_cap), obo.data_ptr(), inf.data_ptr(), ws.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(pt[1], oo) and torch.equal(bt[1], obo) and torch.equal(info, inf)
    n, m = int(oo[-1]), int(obo[-1])
    assert n > n_total - 4000 and int(inf[:, 2].sum()) > 0
    assert torch.equal(pt[0][:n], out[:n]) and torch.equal(bt[0][:m], ob[:m])
    assert (bt[0][:m, 7] != 0).all()


def _once_size(rng, n_points=100000, c=5):
    from pdanet_amd import data_augmentor as da
    names = ["Car", "Pedestrian", "Cyclist"]
    boxes, points = _small_db(rng, names, n_each=40, c=c)
    for n in names:                                            # ONCE extent
        boxes[n][:, 0] = rng.uniform(-60, 60, len(boxes[n]))
        boxes[n][:, 1] = rng.uniform(-60, 60, len(boxes[n]))
    db = da.GtDatabase.from_arrays(names, boxes, points)
    scenes, sboxes, scls = [], [], []
    for b in range(2):
        p, bx = _random_scene(rng, n_points, 12, c=c, id0=b * n_points, extent=60.0)
        scenes.append(p)
        sboxes.append(bx)
        scls.append(rng.integers(0, 4, 12).astype(np.int32))
    cfg = {"DISABLE_AUG_LIST": [], "AUG_CONFIG_LIST": [
        {"NAME": "gt_sampling", "USE_ROAD_PLANE": False, "DB_INFO_PATH": [], "PREPARE": {}, "SAMPLE_GROUPS": ["Car:15", "Pedestrian:15", "Cyclist:15"],
         "NUM_POINT_FEATURES": c, "REMOVE_EXTRA_WIDTH": [0.0, 0.0, 0.0], "LIMIT_WHOLE_SCENE": False}] + FULL_LIST}
    return da.DataAugmentor(cfg, names, db), db, scenes, sboxes, scls


@pytest.mark.gpu
def test_default_plan_invariants_at_once_size():
    rng = np.random.default_rng(5)
    aug, db, scenes, sboxes, scls = _once_size(rng)
    torch.manual_seed(3)
    pt, bt, info = aug(scenes, sboxes, scls)
    P, Bx, info = _unpack(pt, bt, info)
    src = {int(-q[4]): q[3] for q in db.points.cpu().numpy()}
    for b in range(2):
        assert info[b, 0] == len(P[b]) > 50000 and info[b, 1] == len(Bx[b]) > 0 and info[b, 3] == 0 and info[b, 2] > 0
        ids = P[b][:, 4].astype(np.int64)
        assert len(np.unique(ids)) == len(ids)                                          # every output point comes from one source point
        own = ids >= 0
        assert np.array_equal(ids[own], np.sort(ids[own])) and ids[own].min() >= b * 100000 and ids[own].max() < (b + 1) * 100000
        assert np.array_equal(P[b][own, 3], scenes[b][ids[own] - b * 100000, 3])         # ... an input point, in order
        assert all(src[int(-i)] == v for i, v in zip(ids[~own], P[b][~own, 3]))         # ... or a database point
        assert (~own).sum() > 0 and np.isfinite(P[b]).all() and np.isfinite(Bx[b]).all()
        assert ((Bx[b][:, 6] >= f32(-np.pi)) & (Bx[b][:, 6] < f32(np.pi))).all()
        assert (Bx[b][:, 7] >= 1).all()                                                 # no box of class 0 survives


@pytest.mark.gpu
def test_no_host_read_with_device_inputs():
    rng = np.random.default_rng(8)
    aug, db, scenes, sboxes, scls = _once_size(rng, n_points=20000)
    packed = torch.from_numpy(np.concatenate(scenes)).cuda()
    offs = torch.tensor([0, len(scenes[0]), len(scenes[0]) + len(scenes[1])], dtype=torch.int64, device="cuda")
    bx = torch.from_numpy(np.concatenate(sboxes)).cuda()
    boffs = torch.tensor([0, len(sboxes[0]), len(sboxes[0]) + len(sboxes[1])], dtype=torch.int64, device="cuda")
    torch.manual_seed(4)
    ref = aug((packed, offs, 20000), (bx, boffs), scls)                                   # loads the kernels
    torch.cuda.synchronize()
    torch.manual_seed(4)
    aug2 = _once_size(np.random.default_rng(8), n_points=20000)[0]
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = aug2((packed, offs, 20000), (bx, boffs), scls, check=False)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.equal(out[0][1], ref[0][1]) and torch.equal(out[1][1], ref[1][1]) and torch.equal(out[2], ref[2])
    n = int(ref[0][1][-1])
    assert n > 0 and torch.equal(out[0][0][:n], ref[0][0][:n])


@pytest.mark.gpu
def test_kitti_training_iteration_on_program_augmented_scenes():
    """The program's output goes straight into DataProcessor and a KITTI training iteration runs on it."""
    from pdanet_amd import data_augmentor as da, data_processor as dpm, detector
    rng = np.random.default_rng(9)
    names = ["Car", "Pedestrian", "Cyclist"]
    boxes, points = _small_db(rng, names)
    db = da.GtDatabase.from_arrays(names, boxes, points)
    torch.manual_seed(7)
    model, cfg = detector.build_detector("kitti_pda_ssd.yaml")
    model = model.cuda().train()
    aug_cfg = cfg["DATA_CONFIG"]["DATA_AUGMENTOR"]
    steps = [c for c in aug_cfg["AUG_CONFIG_LIST"] if c["NAME"] not in list(aug_cfg.get("DISABLE_AUG_LIST", []))]
    gts = dict(steps[0], USE_ROAD_PLANE=False)
    extra = [c for c in FULL_LIST if c["NAME"].startswith("random_local") or c["NAME"] == "random_world_translation"]
    extra.append({"NAME": "random_world_frustum_dropout", "INTENSITY_RANGE": [0, 0.05], "DIRECTION": ["top"]})
    aug = da.DataAugmentor([gts] + extra[:2] + steps[1:] + extra[2:], names, db)
    assert aug.program is not None and steps[0]["NAME"] == "gt_sampling"
    dp = dpm.from_config(cfg, training=True)
    scenes = [rng.uniform([2, -38, -2.5, 0], [68, 38, 0.5, 1], (n, 4)).astype(f32) for n in (30000, 18000)]
    sb = [np.array([[20.0, 5.0, -0.9, 3.9, 1.6, 1.5, 0.3]], f32), np.zeros((0, 7), f32)]
    pt, bt, info = aug(scenes, sb, [np.array([1], np.int32), np.zeros(0, np.int32)])
    assert (info[:, 2] > 0).all().item() and (info[:, 3] == 0).all().item()
    bd = dp(pt, bt, max_gt=64, seed=5)
    ret, tb, _ = model(bd)
    assert torch.isfinite(ret["loss"])
    ret["loss"].backward()
    assert (bd["gt_boxes"][..., 7] > 0).any().item()
