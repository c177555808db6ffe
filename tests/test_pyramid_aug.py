"""random_local_pyramid_aug on the device (pdanet_amd/data_augmentor.py, csrc/augment_steps.hip: a hold op at the end of
pda_augment_steps, then pda_pyramid_aug) against the float32 restatement of the device contract
(tests/golden/pyramid_aug_restatement.py) and the reference's scenes recorded in tests/golden/pyramid_aug.npz
(tests/golden/make_pyramid_aug_golden.py)."""
import ctypes
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import pyramid_aug_restatement as rs  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "pyramid_aug.npz")
i64 = ctypes.c_int64
f32 = np.float32
NAMES = ["Car", "Pedestrian", "Cyclist"]
COVER = ("dropped", "thinned", "selected_not_thinned", "real_swap", "self_swap", "no_face")
# Swapped rows, restatement against the reference, in float32 steps of the row's largest magnitude: the worst measured on
# the fixture is 1.00.  The bound is twice that: the reference's corners go through a torch matmul whose rounding the
# project already allows 4 steps a rotation for.
SWAP_STEPS = 2.0
# the DATA_AUGMENTOR block of the reference's tools/cfgs/kitti_models/pointpillar_pyramid_aug.yaml
YAML_BLOCK = {"DISABLE_AUG_LIST": ["placeholder"], "AUG_CONFIG_LIST": [
    {"NAME": "gt_sampling", "USE_ROAD_PLANE": True, "DB_INFO_PATH": ["kitti_dbinfos_train.pkl"],
     "PREPARE": {"filter_by_min_points": ["Car:5", "Pedestrian:5", "Cyclist:5"], "filter_by_difficulty": [-1]},
     "SAMPLE_GROUPS": ["Car:15", "Pedestrian:15", "Cyclist:15"], "NUM_POINT_FEATURES": 4, "DATABASE_WITH_FAKELIDAR": False,
     "REMOVE_EXTRA_WIDTH": [0.0, 0.0, 0.0], "LIMIT_WHOLE_SCENE": False},
    {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x"]},
    {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
    {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [0.95, 1.05]},
    {"NAME": "random_local_pyramid_aug", "DROP_PROB": 0.25, "SPARSIFY_PROB": 0.05, "SPARSIFY_MAX_NUM": 50, "SWAP_PROB": 0.1,
     "SWAP_MAX_NUM": 50}]}
PYRAMID = YAML_BLOCK["AUG_CONFIG_LIST"][-1]
DRAW_KEYS = ("drop_face", "drop_u", "sparsify_face", "sparsify_u", "swap_u", "swap_face", "swap_partner")


def _ulps(a, b):
    """|a - b| in float32 steps of the row's largest magnitude (tests/test_augment_steps.py _ulps)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    scale = np.maximum(np.abs(a), np.abs(b)).max(axis=-1, keepdims=True)
    return np.abs(a.astype(np.float64) - b) / np.spacing(scale + f32(1e-30))


def _golden():
    g = dict(np.load(GOLDEN))
    g["cfg"] = dict(zip([str(k) for k in g["cfg_keys"]], g["cfg_values"].tolist()))
    return g


def _step_cfg(g):
    c = g["cfg"]
    return dict(NAME="random_local_pyramid_aug", DROP_PROB=c["DROP_PROB"], SPARSIFY_PROB=c["SPARSIFY_PROB"],
                SPARSIFY_MAX_NUM=int(c["SPARSIFY_MAX_NUM"]), SWAP_PROB=c["SWAP_PROB"], SWAP_MAX_NUM=int(c["SWAP_MAX_NUM"]))


def _rs_cfg(step):
    return dict(drop_prob=step["DROP_PROB"], sparsify_prob=step["SPARSIFY_PROB"], sparsify_max=step["SPARSIFY_MAX_NUM"],
                swap_prob=step["SWAP_PROB"], swap_max=step["SWAP_MAX_NUM"])


def _case(g, tag):
    """points, boxes (m, 7), class ids, the scene's draws as the restatement takes them"""
    from pdanet_amd import data_augmentor as da
    d = {k: g[tag + "_" + k] for k in DRAW_KEYS}
    at = np.concatenate([[0], np.cumsum(g[tag + "_keep_len"])])
    d["sparsify_keep"] = [g[tag + "_keep"][at[j]:at[j + 1]] for j in range(len(at) - 1)]
    return g[tag + "_points"], g[tag + "_boxes"], da.class_ids([str(n) for n in g[tag + "_names"]], NAMES), d


def _plan(draws, extra=None):
    """Per-scene draws of the restatement -> the augmentor's plan."""
    keys = set().union(*[set(d) for d in draws])
    plan = {"pyramid_" + k: [d.get(k, np.zeros(0)) if k != "sparsify_keep" else d.get(k, []) for d in draws] for k in keys}
    plan.update(extra or {})
    return plan


def _boxes8(bx, cls):
    return np.concatenate([np.asarray(bx, f32).reshape(-1, 7), np.asarray(cls, f32).reshape(-1, 1)], 1)


def _compare_with_reference(g, tag, P, src):
    """The scene P, whose row i came from input row src[i], against the reference's: the same set of input rows; rows the
    reference left alone bit for bit; rows it rebuilt (swapped 1, a self pair 2) within SWAP_STEPS."""
    ref, rsrc, flag = g[tag + "_ref_points"], g[tag + "_ref_src"].astype(np.int64), g[tag + "_ref_flag"]
    assert len(set(src.tolist())) == len(src) and sorted(src.tolist()) == sorted(rsrc.tolist()), tag
    order = np.argsort(rsrc)
    at = order[np.searchsorted(rsrc[order], src)]
    ref, flag = ref[at], flag[at]
    assert np.array_equal(P[flag == 0], ref[flag == 0]), tag
    worst = 0.0
    if (flag > 0).any():
        u = _ulps(P[flag > 0], ref[flag > 0])
        worst = float(u.max())
        assert worst <= SWAP_STEPS, (tag, worst)
    return worst


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_fixture_covers_the_cases():
    g = _golden()
    tags = [str(t) for t in g["tags"]]
    assert tags == ["main", "swap2", "single", "nobox", "alldrop", "paste"] and os.path.getsize(GOLDEN) < 1 << 20
    cover = {t: dict(zip(COVER, g[t + "_cover"].tolist())) for t in tags}
    m = cover["main"]
    assert m["dropped"] and m["thinned"] and m["selected_not_thinned"] and m["real_swap"] and m["no_face"]
    assert cover["single"]["self_swap"] == 1 and len(g["single_boxes"]) == 1
    assert len(g["nobox_boxes"]) == 0 and cover["alldrop"]["dropped"] == len(g["alldrop_boxes"]) > 0
    assert g["cfg"]["SPARSIFY_MAX_NUM"] == 8 and g["cfg"]["SWAP_MAX_NUM"] == 8 and g["main_points"].shape[1] == 4
    # the four big boxes hold 150-300 points each, spread over the scene's tiles of 256; a class-0 box holds points
    p, bx, cls, _ = _case(g, "main")
    inside = [np.nonzero(rs.faces(p, b) >= 0)[0] for b in bx]
    assert all(150 <= len(r) <= 300 and len(set(r // 256)) >= 4 for r in inside[:4])
    assert (cls == 0).sum() == 1 and len(inside[int(np.nonzero(cls == 0)[0][0])]) > 0
    assert (g["main_ref_flag"] == 1).any() and (g["single_ref_flag"] == 2).any()
    # gt_sampling in front: a rejected and several accepted candidates, a class-0 box, and pasted boxes in every sub-step
    n_own, n_acc = len(g["paste_raw_boxes"]), int(g["paste_n_accepted"])
    assert 2 <= n_acc < len(g["paste_cand"]) and len(g["paste_boxes"]) == n_own + n_acc and "Van" in g["paste_raw_names"].tolist()
    assert np.array_equal(g["paste_boxes"][:n_own], g["paste_raw_boxes"]) and len(g["paste_points"]) > len(g["paste_raw_points"])
    _, bx, cls, d = _case(g, "paste")
    left1 = [i for i in range(len(bx)) if not d["drop_u"][i] <= g["cfg"]["DROP_PROB"]]
    left2 = [i for j, i in enumerate(left1) if not d["sparsify_u"][j] <= g["cfg"]["SPARSIFY_PROB"]]
    assert any(i >= n_own and i not in left1 for i in range(len(bx)))                                    # a pasted box dropped
    assert any(left1[j] >= n_own for j, k in enumerate(d["sparsify_keep"]) if len(k))                    # a pasted pyramid thinned
    assert any((left2[k] >= n_own) != (left2[q] >= n_own) for k, q in enumerate(d["swap_partner"]) if q >= 0)   # scene <-> pasted


def test_restatement_gives_the_reference_scenes():
    g = _golden()
    cfg = _rs_cfg(_step_cfg(g))
    worst = 0.0
    for tag in [str(t) for t in g["tags"]]:
        p, bx, cls, d = _case(g, tag)
        P, Bx, tr = rs.pyramid_aug(p, _boxes8(bx, cls), cfg, d)
        assert not tr["bad"] and len(P) <= len(p)
        cov = dict(zip(COVER, g[tag + "_cover"].tolist()))
        assert tr["dropped"] == cov["dropped"] and tr["thinned"] == cov["thinned"] and tr["no_face"] == cov["no_face"]
        assert tr["selected_not_thinned"] == cov["selected_not_thinned"]
        assert sum(a for *_, a in tr["pairs"]) == cov["real_swap"] and sum(i == q for i, _, q, _ in tr["pairs"]) == cov["self_swap"]
        assert np.array_equal(Bx[:, :6], bx[cls != 0][:, :6]) and np.array_equal(Bx[:, 7], cls[cls != 0].astype(f32))
        assert np.array_equal(tr["moved"], g[tag + "_ref_flag"][np.argsort(g[tag + "_ref_src"])] == 1)
        worst = max(worst, _compare_with_reference(g, tag, P, tr["src"]))
    print("swapped rows against the reference: worst %.2f float32 steps (bound %.1f)" % (worst, SWAP_STEPS))


def _cpu_db(rng=None):
    from pdanet_amd import data_augmentor as da
    rng = rng or np.random.default_rng(1)
    boxes = {n: np.concatenate([rng.uniform([2, -6, -1], [11, 6, -0.5], (4, 3)), np.tile([1.6, 0.8, 1.5, 0.3], (4, 1))], 1) for n in NAMES}
    points = {n: [np.concatenate([rng.uniform(-0.4, 0.4, (120, 3)) * b[3:6], rng.random((120, 1))], 1).astype(f32) for b in boxes[n]]
              for n in NAMES}
    return boxes, points, lambda device: da.GtDatabase.from_arrays(NAMES, boxes, points, device=device)


def test_construction_rules():
    from pdanet_amd import data_augmentor as da
    db = _cpu_db()[2]("cpu")
    aug = da.from_config({"CLASS_NAMES": NAMES, "DATA_CONFIG": {"DATA_AUGMENTOR": YAML_BLOCK}}, db)
    assert aug.pyramid == dict(drop_prob=0.25, sparsify_prob=0.05, sparsify_max=50, swap_prob=0.1, swap_max=50)
    assert [st[0] for st in aug.program] == [da.OP_FLIP_X, da.OP_ROT, da.OP_SCALE]          # the op codes of the steps stay 0..9
    assert da.DataAugmentor([PYRAMID], NAMES).program == []
    for key in ("DROP_PROB", "SPARSIFY_PROB", "SPARSIFY_MAX_NUM", "SWAP_PROB", "SWAP_MAX_NUM"):
        with pytest.raises(NotImplementedError) as e:
            da.DataAugmentor([{k: v for k, v in PYRAMID.items() if k != key}], NAMES)
        assert "random_local_pyramid_aug" in str(e.value) and key in str(e.value)
    with pytest.raises(NotImplementedError, match="twice"):
        da.DataAugmentor([PYRAMID, PYRAMID], NAMES)
    with pytest.raises(NotImplementedError, match="last"):                                  # only the yaml's place is supported
        da.DataAugmentor([PYRAMID, {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x"]}], NAMES)
    with pytest.raises(ValueError):
        da.DataAugmentor([dict(PYRAMID, SPARSIFY_MAX_NUM=5000)], NAMES)
    # a disabled entry is not looked at
    assert da.DataAugmentor({"DISABLE_AUG_LIST": ["random_local_pyramid_aug"], "AUG_CONFIG_LIST": [
        {"NAME": "random_local_pyramid_aug"}, {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x"]}]}, NAMES).pyramid is None


def test_make_plan_shapes_and_reproducibility():
    from pdanet_amd import data_augmentor as da
    cls = [np.array([1, 0, 2], np.int32), np.zeros(0, np.int32)]

    def plan(seed):
        torch.manual_seed(seed)
        return da.DataAugmentor(YAML_BLOCK, NAMES, _cpu_db()[2]("cpu")).make_plan(cls)

    p, q, r = plan(3), plan(3), plan(4)
    D = max(len(cls[b]) + len(p["cand"][b]) for b in range(2))
    keys = ("pyramid_drop_face", "pyramid_drop_u", "pyramid_sparsify_face", "pyramid_sparsify_u", "pyramid_sparsify_key",
            "pyramid_swap_u", "pyramid_swap_face_u", "pyramid_swap_partner_u")
    for k in keys:
        assert p[k].shape == (2, D) and np.array_equal(p[k], q[k]), k
    assert p["pyramid_sparsify_key"].dtype == np.uint64 and not np.array_equal(p["pyramid_drop_u"], r["pyramid_drop_u"])
    for k in ("pyramid_drop_face", "pyramid_sparsify_face"):
        assert ((p[k] >= 0) & (p[k] <= 5)).all()
    for k in ("pyramid_drop_u", "pyramid_sparsify_u", "pyramid_swap_u", "pyramid_swap_face_u", "pyramid_swap_partner_u"):
        assert ((p[k] >= 0) & (p[k] < 1)).all()
    aug = da.DataAugmentor([PYRAMID], NAMES)
    one = dict(drop_face=[1, 2], drop_u=[0.1, 0.9], sparsify_face=[3], sparsify_u=[0.5], swap_u=[0.7], sparsify_keep=[[1, 2, 3]])
    f64, i32, keys_, keep, n, D2 = aug._pyramid_draws(_plan([one]), 1)
    assert D2 == 2 and n.tolist() == [[2, 1, 1]] and f64.shape == (1, 5, 2) and i32.shape == (1, 4, 2) and keep.shape == (1, 2, 51)
    assert i32[0, 0].tolist() == [1, 2] and i32[0, 2].tolist() == [-1, -1] and keep[0, 0, :4].tolist() == [3, 1, 2, 3]
    with pytest.raises(ValueError, match="lacks"):
        aug._pyramid_draws({"pyramid_drop_u": [[0.5]]}, 1)


@pytest.fixture(scope="module")
def lib():
    from pdanet_amd import build, _lib
    build.build()
    return _lib.load()


def test_argument_validation_without_gpu(lib):
    assert lib.pda_abi_version() == 20
    assert lib.pda_pyramid_aug_workspace_bytes(2, i64(1000), 40) > 0
    assert lib.pda_pyramid_aug_workspace_bytes(0, i64(1000), 0) >= 0
    assert lib.pda_pyramid_aug_workspace_bytes(-1, i64(1000), 40) == -1
    assert lib.pda_pyramid_aug_workspace_bytes(2, i64(0), 40) == -1
    assert lib.pda_pyramid_aug_workspace_bytes(2, i64(1000), 257) == -1
    probs = (ctypes.c_double * 3)(0.5, 0.5, 0.5)

    def call(batch=2, c=4, n_cap=10, draw_cap=4, slots=4, smax=8, wmax=8, out_cap=0, probs=probs):
        return lib.pda_pyramid_aug(None, None, i64(0), batch, c, i64(n_cap), None, None, i64(0), None, None, None, None, None, draw_cap,
                                   probs, smax, wmax, slots, None, None, i64(out_cap), None, None, i64(0), None, None, None, None)

    assert call(batch=0) == 0
    for bad in (dict(c=3), dict(n_cap=0), dict(draw_cap=257), dict(slots=300), dict(smax=-1), dict(smax=1025), dict(wmax=-1), dict(out_cap=-1)):
        assert call(**bad) == 1 and b"pda_pyramid_aug: bad size" in lib.pda_last_error(), bad
    assert call(probs=None) == 1 and b"null" in lib.pda_last_error()
    assert call() == 1 and b"null" in lib.pda_last_error()
    # the hold op of pda_augment_steps is the last op or none
    ops = (ctypes.c_int32 * 4)(0, 0, 10, 0)

    def steps(ops, n_ops, batch=2):
        return lib.pda_augment_steps(None, None, i64(0), batch, 4, i64(10), None, None, i64(0), ops, n_ops, None, None, 0, 4, None, None,
                                     i64(0), None, None, i64(0), None, None, None, None)

    assert steps(ops, 2, batch=0) == 0
    assert steps((ctypes.c_int32 * 4)(10, 0, 0, 0), 2) == 1 and b"bad op" in lib.pda_last_error()
    assert steps((ctypes.c_int32 * 2)(10, 1), 1) == 1 and b"bad op" in lib.pda_last_error()


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _run(aug, scenes, boxes, classes, plan, check=True):
    pt, bt, info = aug(scenes, boxes, classes, plan=plan, check=check)
    o, bo = pt[1].cpu().numpy(), bt[1].cpu().numpy()
    P, Bx = pt[0].cpu().numpy(), bt[0].cpu().numpy()
    return [P[o[b]:o[b + 1]] for b in range(len(o) - 1)], [Bx[bo[b]:bo[b + 1]] for b in range(len(bo) - 1)], info.cpu().numpy()


@pytest.mark.gpu
def test_recorded_draws_give_the_restatement_and_the_reference_scenes():
    """All fixture scenes as one batch: point order, every row and the boxes bit for bit against the restatement (the
    device's (float)cos((double)) agreed with the host's on every box of the fixture), then the reference comparison of the
    CPU test on the device output."""
    from pdanet_amd import data_augmentor as da
    g = _golden()
    step = _step_cfg(g)
    tags = [str(t) for t in g["tags"]]
    cases = [_case(g, t) for t in tags]
    aug = da.DataAugmentor([step], NAMES)
    P, Bx, info = _run(aug, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], _plan([c[3] for c in cases]))
    for b, (tag, (p, bx, cls, d)) in enumerate(zip(tags, cases)):
        wP, wB, tr = rs.pyramid_aug(p, _boxes8(bx, cls), _rs_cfg(step), d)
        assert P[b].shape == wP.shape, tag
        assert np.array_equal(P[b][~tr["moved"]], wP[~tr["moved"]]), tag
        assert np.array_equal(P[b][tr["moved"]], wP[tr["moved"]]), tag
        assert np.array_equal(Bx[b], wB), tag
        assert info[b].tolist() == [len(wP), len(wB), 0, 0 if len(wB) and len(wP) else da.STATUS_NO_BOX], tag
        _compare_with_reference(g, tag, P[b], tr["src"])


@pytest.mark.gpu
def test_gt_sampling_in_front_gives_the_restatement_and_the_reference_scene(tmp_path):
    """The `paste` case from its raw scene: gt_sampling with the recorded candidates, the hold, then all three sub-steps
    with the recorded draws on scene, class-0 and pasted boxes.  The output is the restatement's on the reference's pasted
    scene bit for bit, and the reference's scene within the bound of the CPU comparison."""
    from pdanet_amd import data_augmentor as da
    g = _golden()
    cfg = pickle.loads(g["paste_aug_cfg"].item())
    infos = pickle.loads(g["paste_dbinfos"].item())
    off = g["paste_db_point_offsets"]
    os.makedirs(os.path.join(str(tmp_path), "gt_database"), exist_ok=True)
    with open(os.path.join(str(tmp_path), "dbinfos.pkl"), "wb") as f:
        pickle.dump(infos, f)
    for k, path in enumerate(str(x) for x in g["paste_db_paths"]):
        g["paste_db_points"][off[k]:off[k + 1]].tofile(os.path.join(str(tmp_path), path))
    db = da.GtDatabase.from_dbinfos(str(tmp_path), cfg["AUG_CONFIG_LIST"][0], NAMES, device="cuda")
    aug = da.DataAugmentor(cfg, NAMES, db)
    assert aug.pyramid is not None and aug.program == [] and aug.groups
    p, bx, cls, d = _case(g, "paste")
    raw_cls = da.class_ids([str(n) for n in g["paste_raw_names"]], NAMES)
    plan = _plan([d], dict(cand=[g["paste_cand"]], cand_group=[g["paste_cand_group"]]))
    P, Bx, info = _run(aug, [g["paste_raw_points"]], [g["paste_raw_boxes"]], [raw_cls], plan)
    step = _step_cfg(g)
    wP, wB, tr = rs.pyramid_aug(p, _boxes8(bx, cls), _rs_cfg(step), d)
    assert tr["moved"].any() and tr["thinned"] and tr["dropped"] and not tr["bad"]
    assert np.array_equal(P[0], wP) and np.array_equal(Bx[0], wB)
    assert info[0].tolist() == [len(wP), len(wB), int(g["paste_n_accepted"]), 0]
    _compare_with_reference(g, "paste", P[0], tr["src"])


def _two_box_scene(rng, overlap, c=4, n_each=120, n_bg=200):
    """Two boxes of n_each points each (the second shifted into the first when `overlap`), every pyramid well above 8."""
    bx = np.array([[10, 0, -0.8, 4.0, 1.8, 1.6, 0.4], [10.8 if overlap else 20, 0.3, -0.8, 4.2, 1.7, 1.6, -0.5 if overlap else 2.0]], f32)
    rows = []
    for b in bx:
        loc = rng.uniform(-0.5, 0.5, (n_each, 3)) * b[3:6]
        cs, sn = np.cos(b[6]), np.sin(b[6])
        rows.append(np.stack([loc[:, 0] * cs - loc[:, 1] * sn + b[0], loc[:, 0] * sn + loc[:, 1] * cs + b[1], loc[:, 2] + b[2]], 1))
    rows.append(np.concatenate([rng.uniform([0, -10], [30, 10], (n_bg, 2)), rng.uniform(-2, 0, (n_bg, 1))], 1))
    xyz = np.concatenate(rows)[rng.permutation(2 * n_each + n_bg)]
    p = np.concatenate([xyz, rng.random((len(xyz), c - 3))], 1).astype(f32)
    return p, bx


NO_DROP = dict(NAME="random_local_pyramid_aug", DROP_PROB=0.0, SPARSIFY_PROB=0.0, SPARSIFY_MAX_NUM=8, SWAP_PROB=0.5, SWAP_MAX_NUM=8)


def _swap_draws(m, swap_u, face=None, partner=None):
    d = dict(drop_face=np.zeros(m, np.int32), drop_u=np.ones(m), sparsify_face=np.zeros(m, np.int32), sparsify_u=np.ones(m),
             swap_u=np.asarray(swap_u, np.float64))
    if face is not None:
        d["swap_face"] = np.asarray(face, np.int32)
    if partner is not None:
        d["swap_partner"] = np.asarray(partner, np.int32)
    return d


@pytest.mark.gpu
def test_departures_are_known_answers():
    """A contested partner, two overlapping boxes and C = 5 against the restatement; no scene grows."""
    from pdanet_amd import data_augmentor as da
    rng = np.random.default_rng(31)
    aug = da.DataAugmentor([NO_DROP], NAMES)
    # three boxes, boxes 0 and 1 both swap face 0 with box 2: the second pair does nothing
    p0, b2 = _two_box_scene(rng, False, n_each=150)
    third = np.array([[15, 6, -0.8, 4.0, 1.8, 1.6, 1.0]], f32)
    loc = rng.uniform(-0.5, 0.5, (150, 3)) * third[0, 3:6]
    q = np.stack([loc[:, 0] * np.cos(1.0) - loc[:, 1] * np.sin(1.0) + 15, loc[:, 0] * np.sin(1.0) + loc[:, 1] * np.cos(1.0) + 6, loc[:, 2] - 0.8], 1)
    p0 = np.concatenate([p0, np.concatenate([q, rng.random((150, 1))], 1).astype(f32)])[rng.permutation(len(p0) + 150)]
    b3 = np.concatenate([b2, third])
    d0 = _swap_draws(3, [0.1, 0.1, 0.9], face=[0, 0, -1], partner=[2, 2, -1])
    # two overlapping boxes, box 0 swaps face 0 with box 1: a point in both pyramids is moved once
    p1, b1 = _two_box_scene(rng, True)
    d1 = _swap_draws(2, [0.1, 0.9], face=[0, -1], partner=[1, -1])
    cls = [np.array([1, 2, 1], np.int32), np.array([1, 1], np.int32)]
    P, Bx, info = _run(aug, [p0, p1], [b3, b1], cls, _plan([d0, d1]))
    for b, (p, bx, d) in enumerate(((p0, b3, d0), (p1, b1, d1))):
        wP, wB, tr = rs.pyramid_aug(p, _boxes8(bx, cls[b]), _rs_cfg(NO_DROP), d)
        assert not tr["bad"] and len(P[b]) == len(p) == len(wP) and tr["moved"].any()
        assert np.array_equal(P[b], wP) and np.array_equal(Bx[b], wB)
    assert rs.pyramid_aug(p0, _boxes8(b3, cls[0]), _rs_cfg(NO_DROP), d0)[2]["pairs"] == [(0, 0, 2, True), (1, 0, 2, False)]
    f0, f1 = rs.faces(p1, b1[0]), rs.faces(p1, b1[1])
    assert ((f0 == 0) & (f1 == 0)).any()                                                # a point in both pyramids of the pair
    # C = 5: xyz and the last column are rewritten, the middle column travels with the point
    p5, b5 = _two_box_scene(rng, False, c=5)
    d5 = _swap_draws(2, [0.1, 0.9], face=[1, -1], partner=[1, -1])
    P, Bx, info = _run(aug, [p5], [b5], [cls[1]], _plan([d5]))
    wP, wB, tr = rs.pyramid_aug(p5, _boxes8(b5, cls[1]), _rs_cfg(NO_DROP), d5)
    assert np.array_equal(P[0], wP) and tr["moved"].sum() > 16 and len(wP) == len(p5)
    assert np.array_equal(P[0][:, 3], p5[:, 3]) and (P[0][tr["moved"]][:, 4] != p5[tr["moved"]][:, 4]).any()


@pytest.mark.gpu
def test_invalid_explicit_draws_flag_the_scene():
    from pdanet_amd import data_augmentor as da
    rng = np.random.default_rng(32)
    p, bx = _two_box_scene(rng, False)
    cls = np.array([1, 1], np.int32)
    good = _swap_draws(2, [0.1, 0.9], face=[0, -1], partner=[1, -1])
    sp = dict(good, sparsify_u=np.array([0.0, 1.0]), swap_u=np.array([0.9]), swap_face=np.array([-1], np.int32),
              swap_partner=np.array([-1], np.int32))
    cfg = dict(NO_DROP, SPARSIFY_PROB=0.5)
    aug = da.DataAugmentor([cfg], NAMES)
    bad = [dict(sp, sparsify_keep=[[0, 1, 2, 3, 4, 5, 6, 6]]),                            # a repeated keep rank
           dict(sp, sparsify_keep=[[0, 1, 2, 3, 4, 5, 6, 500]]),                          # a rank out of range
           dict(sp, sparsify_keep=[[0, 1, 2]]),                                           # a keep list of the wrong length
           dict(good, swap_face=np.array([6, -1], np.int32)),                             # no such face
           dict(good, swap_partner=np.array([0, -1], np.int32)),                          # the box itself while a candidate exists
           dict(good, drop_u=np.ones(1), drop_face=np.zeros(1, np.int32)),                # a short row
           dict(good, swap_partner=np.array([5, -1], np.int32)),                          # a partner beyond the boxes left
           good,                                                                          # scene 7: face 0 of box 0 holds no point
           dict(good, swap_face=np.array([2, -1], np.int32)),                             # scene 8: box 1 is no candidate for face 2
           dict(sp, sparsify_keep=[[7, 6, 5, 4, 3, 2, 1, 0]]), good]                      # two valid scenes
    n = len(bad)
    scenes = [p] * n
    scenes[7] = p[rs.faces(p, bx[0]) != 0]                  # the explicit face 0 is a face, but without count > SWAP_MAX_NUM
    scenes[8] = p[rs.faces(p, bx[1]) != 2]                  # no candidate at all for face 2: the only valid partner is box 0 itself
    P, Bx, info = _run(aug, scenes, [bx] * n, [cls] * n, _plan(bad), check=False)
    for b, d in enumerate(bad):
        p = scenes[b]
        wP, wB, tr = rs.pyramid_aug(p, _boxes8(bx, cls), _rs_cfg(cfg), d)
        assert tr["bad"] == (b < n - 2), b
        if tr["bad"]:
            assert info[b].tolist() == [0, 0, 0, da.STATUS_BAD_PYRAMID_DRAW | da.STATUS_NO_BOX] and len(P[b]) == 0 and len(Bx[b]) == 0, b
        else:
            assert info[b, 3] == 0 and np.array_equal(P[b], wP) and np.array_equal(Bx[b], wB), b
    with pytest.raises(ValueError, match="random_local_pyramid_aug"):
        aug([p], [bx], [cls], plan=_plan(bad[:1]))


def _many_boxes(rng, m, per_box):
    """m boxes on a grid, per_box points in each, interleaved."""
    g = int(np.ceil(np.sqrt(m)))
    ctr = np.stack([6.0 * (np.arange(m) % g), 6.0 * (np.arange(m) // g), np.full(m, -0.8)], 1)
    bx = np.concatenate([ctr, np.tile([3.9, 1.6, 1.5], (m, 1)) * rng.uniform(0.9, 1.1, (m, 3)), rng.uniform(-np.pi, np.pi, (m, 1))], 1).astype(f32)
    k = np.repeat(np.arange(m), per_box)
    loc = rng.uniform(-0.5, 0.5, (len(k), 3)) * bx[k, 3:6]
    c, s = np.cos(bx[k, 6]), np.sin(bx[k, 6])
    xyz = np.stack([loc[:, 0] * c - loc[:, 1] * s + bx[k, 0], loc[:, 0] * s + loc[:, 1] * c + bx[k, 1], loc[:, 2] + bx[k, 2]], 1)
    p = np.concatenate([xyz, rng.random((len(k), 1))], 1).astype(f32)
    return p[rng.permutation(len(p))], bx


@pytest.mark.gpu
def test_seeded_mode():
    """400 boxes in two scenes, the draws from make_plan: every thinned pyramid holds exactly SPARSIFY_MAX_NUM points, a
    seed gives its scene again, another seed another subset, and the dropped share follows DROP_PROB."""
    from pdanet_amd import data_augmentor as da
    rng = np.random.default_rng(33)
    cfg = dict(NAME="random_local_pyramid_aug", DROP_PROB=0.3, SPARSIFY_PROB=0.5, SPARSIFY_MAX_NUM=8, SWAP_PROB=0.0, SWAP_MAX_NUM=8)
    scenes = [_many_boxes(rng, 200, 120) for _ in range(2)]
    cls = [np.ones(200, np.int32)] * 2
    aug = da.DataAugmentor([cfg], NAMES)

    def run(seed):
        torch.manual_seed(seed)
        plan = aug.make_plan(cls)
        return plan, _run(aug, [s[0] for s in scenes], [s[1] for s in scenes], cls, plan)[0]

    plan, P = run(1)
    assert all(np.array_equal(a, b) for a, b in zip(P, run(1)[1]))
    plan2, P2 = run(2)
    dropped = thinned = 0
    for b, (p, bx) in enumerate(scenes):
        out_rows = {r.tobytes() for r in P[b]}
        keep = np.array([r.tobytes() in out_rows for r in p])
        assert keep.sum() == len(P[b]) and np.array_equal(p[keep], P[b])                 # scene order, nothing moved
        du, su = plan["pyramid_drop_u"][b], plan["pyramid_sparsify_u"][b]
        left = [i for i in range(200) if not du[i] <= 0.3]
        dropped += 200 - len(left)
        for i in range(200):
            f = rs.faces(p, bx[i])
            if du[i] <= 0.3:
                assert not keep[f == plan["pyramid_drop_face"][b][i]].any()
        for j, i in enumerate(left):
            if su[j] <= 0.5:
                f = rs.faces(p, bx[i]) == plan["pyramid_sparsify_face"][b][j]
                if f.sum() > 8:
                    thinned += 1
                    assert keep[f].sum() == 8, (b, i)
                else:
                    assert keep[f].all()
    assert thinned > 50
    sd = np.sqrt(400 * 0.3 * 0.7)
    assert abs(dropped - 400 * 0.3) <= 5 * sd, dropped
    # the same draws with other keys: another kept subset of the same size
    plan3 = dict(plan, pyramid_sparsify_key=plan2["pyramid_sparsify_key"])
    P3 = _run(aug, [s[0] for s in scenes], [s[1] for s in scenes], cls, plan3)[0]
    assert [len(x) for x in P3] == [len(x) for x in P] and not np.array_equal(P3[0], P[0])


@pytest.mark.gpu
def test_seeded_draws_match_the_restatement():
    """make_plan's draws (keys, face and partner u) through all three sub-steps, bit for bit against the restatement."""
    from pdanet_amd import data_augmentor as da
    rng = np.random.default_rng(36)
    cfg = dict(NAME="random_local_pyramid_aug", DROP_PROB=0.3, SPARSIFY_PROB=0.3, SPARSIFY_MAX_NUM=8, SWAP_PROB=0.6, SWAP_MAX_NUM=8)
    scenes = [_many_boxes(rng, m, 150) for m in (14, 9)]
    cls = [rng.integers(0, 3, len(s[1])).astype(np.int32) for s in scenes]
    aug = da.DataAugmentor([cfg], NAMES)
    torch.manual_seed(6)
    plan = aug.make_plan(cls)
    P, Bx, info = _run(aug, [s[0] for s in scenes], [s[1] for s in scenes], cls, plan)
    pairs = []
    for b, (p, bx) in enumerate(scenes):
        d = {k[len("pyramid_"):]: v[b] for k, v in plan.items() if k.startswith("pyramid_")}
        wP, wB, tr = rs.pyramid_aug(p, _boxes8(bx, cls[b]), _rs_cfg(cfg), d)
        assert np.array_equal(P[b], wP) and np.array_equal(Bx[b], wB) and not tr["bad"]
        assert info[b].tolist() == [len(wP), len(wB), 0, 0]
        pairs += tr["pairs"]
    assert sum(a for *_, a in pairs) >= 2 and tr["thinned"] + tr["dropped"] > 0


def _gpu_db():
    boxes, points, make = _cpu_db(np.random.default_rng(2))
    return make("cuda")


@pytest.mark.gpu
def test_pasted_and_class0_boxes_take_part():
    """gt_sampling in front, no world step, DROP_PROB 1 with face 0 for every draw: the +x pyramid of every box -- the
    scene's own, the class-0 one and every pasted one -- is empty afterwards, and the other pyramids of the pasted boxes
    still hold their objects' points.  (All headings lie in [-pi, pi), so limit_period leaves the output boxes as they went in.)"""
    from pdanet_amd import data_augmentor as da
    rng = np.random.default_rng(37)
    gts = dict(YAML_BLOCK["AUG_CONFIG_LIST"][0], USE_ROAD_PLANE=False)
    cfg = dict(PYRAMID, DROP_PROB=1.0, SPARSIFY_PROB=0.0, SWAP_PROB=0.0)
    aug = da.DataAugmentor([gts, cfg], NAMES, _gpu_db())
    p, bx = _two_box_scene(rng, False, n_bg=2000)
    cls = [np.array([1, 0], np.int32)]
    torch.manual_seed(8)
    plan = aug.make_plan(cls)
    plan["pyramid_drop_face"] = np.zeros_like(plan["pyramid_drop_face"])
    P, Bx, info = _run(aug, [p], [bx], cls, plan)
    accepted = int(info[0, 2])
    assert accepted > 0 and info[0].tolist() == [len(P[0]), 1 + accepted, accepted, 0] and len(P[0]) > 2000
    assert np.array_equal(Bx[0][0, :7], bx[0])
    for b in list(Bx[0][:, :7]) + [bx[1]]:
        before = rs.faces(p, b)
        f = rs.faces(P[0], b)
        assert not (f == 0).any() and (f > 0).sum() >= 60
        assert (f > 0).sum() >= (before > 0).sum()                                     # pasted points came in, none of these left


@pytest.mark.gpu
def test_no_host_read_with_device_inputs():
    from pdanet_amd import data_augmentor as da
    rng = np.random.default_rng(34)
    steps = [dict(YAML_BLOCK["AUG_CONFIG_LIST"][0], USE_ROAD_PLANE=False)] + YAML_BLOCK["AUG_CONFIG_LIST"][1:-1] + \
            [dict(PYRAMID, SPARSIFY_MAX_NUM=8, SWAP_MAX_NUM=8, SPARSIFY_PROB=0.5, SWAP_PROB=0.5)]
    scenes = [_two_box_scene(rng, False, n_bg=3000) for _ in range(2)]
    packed = torch.from_numpy(np.concatenate([s[0] for s in scenes])).cuda()
    n0 = len(scenes[0][0])
    offs = torch.tensor([0, n0, n0 + len(scenes[1][0])], dtype=torch.int64, device="cuda")
    bx = torch.from_numpy(np.concatenate([s[1] for s in scenes])).cuda()
    boffs = torch.tensor([0, 2, 4], dtype=torch.int64, device="cuda")
    cls = [np.array([1, 0], np.int32), np.array([2, 1], np.int32)]
    torch.manual_seed(4)
    ref = da.DataAugmentor(steps, NAMES, _gpu_db())((packed, offs, 4000), (bx, boffs), cls)           # loads the kernels
    torch.cuda.synchronize()
    torch.manual_seed(4)
    aug2 = da.DataAugmentor(steps, NAMES, _gpu_db())
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = aug2((packed, offs, 4000), (bx, boffs), cls, check=False)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.equal(out[0][1], ref[0][1]) and torch.equal(out[1][1], ref[1][1]) and torch.equal(out[2], ref[2])
    n = int(ref[0][1][-1])
    assert n > 0 and torch.equal(out[0][0][:n], ref[0][0][:n]) and (ref[2][:, 3] == 0).all().item()
    assert (ref[1][0][:int(ref[1][1][-1]), 7] > 0).all().item()                           # class 0 took part and left at the end


@pytest.mark.gpu
def test_pointpillar_training_iteration_on_pyramid_augmented_scenes():
    """The yaml's step list (gt_sampling, flip, rotation, scaling, pyramid aug) feeds a PointPillar training iteration."""
    from pdanet_amd import data_augmentor as da
    from pdanet_amd.config import to_attr
    from pdanet_amd.pointpillar import PointPillar
    from pdanet_amd.voxel_utils import VoxelGenerator, collate_voxels
    G = np.load(os.path.join(HERE, "golden", "anchor_head.npz"))
    c = json.loads(str(G["configs"]))["a"]
    model_cfg = {"NAME": "PointPillar",
                 "VFE": {"NAME": "PillarVFE", "WITH_DISTANCE": False, "USE_ABSLOTE_XYZ": True, "USE_NORM": True, "NUM_FILTERS": [32]},
                 "MAP_TO_BEV": {"NAME": "PointPillarScatter", "NUM_BEV_FEATURES": 32},
                 "BACKBONE_2D": {"NAME": "BaseBEVBackbone", "LAYER_NUMS": [1, 1], "LAYER_STRIDES": [2, 2], "NUM_FILTERS": [32, 64],
                                 "UPSAMPLE_STRIDES": [1, 2], "NUM_UPSAMPLE_FILTERS": [32, 32]},
                 "DENSE_HEAD": dict(c["head"], NAME="AnchorHeadSingle"),
                 "POST_PROCESSING": {"RECALL_THRESH_LIST": [0.3, 0.5, 0.7], "SCORE_THRESH": 0.1, "OUTPUT_RAW_SCORE": False,
                                     "NMS_CONFIG": {"MULTI_CLASSES_NMS": False, "NMS_TYPE": "nms_gpu", "NMS_THRESH": 0.01,
                                                    "NMS_PRE_MAXSIZE": 4096, "NMS_POST_MAXSIZE": 500}}}
    dataset = {"class_names": c["class_names"], "point_cloud_range": c["point_cloud_range"], "voxel_size": c["voxel_size"],
               "num_point_features": 4}
    assert c["class_names"] == NAMES
    torch.manual_seed(3)
    model = PointPillar(to_attr(model_cfg), 3, dataset).cuda().train()
    steps = [dict(YAML_BLOCK["AUG_CONFIG_LIST"][0], USE_ROAD_PLANE=False, SAMPLE_GROUPS=["Car:3", "Pedestrian:2", "Cyclist:2"])] + \
        [dict(YAML_BLOCK["AUG_CONFIG_LIST"][2], WORLD_ROT_ANGLE=[-0.1, 0.1])] + [YAML_BLOCK["AUG_CONFIG_LIST"][3]] + \
        [dict(PYRAMID, SPARSIFY_MAX_NUM=10, SWAP_MAX_NUM=10, SPARSIFY_PROB=0.3, SWAP_PROB=0.5)]
    aug = da.DataAugmentor(steps, NAMES, _gpu_db())
    rng = np.random.default_rng(35)
    pcr = np.array(c["point_cloud_range"], np.float64)
    scenes = [np.concatenate([rng.uniform(pcr[:3], pcr[3:], (n, 3)), rng.random((n, 1))], 1).astype(f32) for n in (1500, 900)]
    sb = [np.array([[6.0, 7.0, -0.9, 1.6, 0.8, 1.5, 0.3]], f32), np.zeros((0, 7), f32)]
    pt, bt, info = aug(scenes, sb, [np.array([1], np.int32), np.zeros(0, np.int32)])
    assert (info[:, 2] > 0).any().item() and (info[:, 3] == 0).all().item()
    gen = VoxelGenerator(c["voxel_size"], c["point_cloud_range"], 4, 32, 2000)
    voxels, coords, num_points = collate_voxels(*gen.generate_batch(pt))
    bo = bt[1].cpu().numpy()
    gt = torch.zeros((2, 16, 8), device="cuda")
    for b in range(2):
        gt[b, :bo[b + 1] - bo[b]] = bt[0][bo[b]:bo[b + 1]]
    ret, tb, _ = model({"voxels": voxels, "voxel_coords": coords, "voxel_num_points": num_points, "gt_boxes": gt, "batch_size": 2})
    assert torch.isfinite(ret["loss"])
    ret["loss"].backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
