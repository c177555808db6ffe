"""Dynamic voxelization (csrc/dyn_voxel.hip, pdanet_amd/dyn_voxel_utils.py, pdanet_amd/dynamic_vfe.py) against
tests/golden/dyn_voxel.npz: the reference's DynamicMeanVFE / DynamicPillarVFE run on the CPU by
tests/golden/make_dyn_voxel_golden.py with a stand-in torch_scatter (torch_scatter itself was not run).  No test reads the
reference."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = (("abs_dist", True, True), ("rel", False, False))      # tag, USE_ABSLOTE_XYZ, WITH_DISTANCE


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(HERE, "golden", "dyn_voxel.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def generator():
    spec = importlib.util.spec_from_file_location("make_dyn_voxel_golden", os.path.join(HERE, "golden", "make_dyn_voxel_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _spec(gold, setting):
    from pdanet_amd.dyn_voxel_utils import DynVoxelSpec
    name = "voxel" if setting == "voxel" else "pillar"
    return DynVoxelSpec(gold[name + "_range"].tolist(), gold[name + "_size"].tolist(), gold[name + "_grid"].tolist())


def _cfg(gold, use_abs, with_dist):
    return {"USE_NORM": True, "WITH_DISTANCE": with_dist, "USE_ABSLOTE_XYZ": use_abs, "NUM_FILTERS": gold["num_filters"].tolist()}


def _pillar_vfe(gold, use_abs, with_dist):
    from pdanet_amd.dynamic_vfe import DynamicPillarVFE
    return DynamicPillarVFE(_cfg(gold, use_abs, with_dist), gold["points"].shape[1] - 1, gold["pillar_size"].tolist(),
                            gold["pillar_grid"].tolist(), gold["pillar_range"].tolist())


def _expected(gold, setting):
    """The padded outputs of the index stage as the fixture gives them."""
    n = len(gold["points"])
    inv, cnt = gold[setting + "_unq_inv"], gold[setting + "_unq_cnt"]
    nk, nv = len(inv), len(cnt)
    pad = lambda a, rows: np.concatenate([a, np.zeros((rows - len(a),) + a.shape[1:], a.dtype)])      # noqa: E731
    return {"counts": np.array([nk, nv], np.int32), "point_idx": pad(gold[setting + "_point_idx"], n), "unq_inv": pad(inv, n),
            "unq_cnt": pad(cnt, n), "voxel_coords": pad(gold[setting + "_coords"] if setting == "pillar" else gold["voxel_coords"], n),
            "seg_points": pad(np.argsort(inv, kind="stable").astype(np.int32), n),
            "seg_start": pad(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), n + 1)}


def _index_np(index):
    return {k: getattr(index, k).cpu().numpy() for k in ("counts", "point_idx", "unq_inv", "unq_cnt", "voxel_coords", "seg_points",
                                                         "seg_start")}


def _run_index(gold, setting, points=None):
    from pdanet_amd.dyn_voxel_utils import dynamic_voxel_index
    pts = torch.from_numpy(gold["points"] if points is None else points).cuda()
    return pts, dynamic_voxel_index(pts, _spec(gold, setting), int(gold["batch"]), pillars=(setting == "pillar"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _f64(gold, key):
    return gold[key].astype(np.float64) + gold[key + "_d64"].astype(np.float64)


# ---- without a GPU -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,use_abs,with_dist", CASES)
def test_state_dict_keys(gold, tag, use_abs, with_dist):
    vfe = _pillar_vfe(gold, use_abs, with_dist)
    state = vfe.state_dict()
    assert list(state.keys()) == gold[tag + "_state_keys"].tolist()
    for k, v in state.items():
        assert tuple(v.shape) == gold["%s_state.%s" % (tag, k)].shape, k
    assert vfe.get_output_feature_dim() == 64
    assert state["pfn_layers.0.linear.weight"].shape[1] == (12 if use_abs else 8)


def test_argument_validation_without_gpu():
    from pdanet_amd import build, _lib
    build.build()
    lib = _lib.load()
    i64, f3, f6, i3 = ctypes.c_int64, ctypes.c_float * 3, ctypes.c_float * 6, ctypes.c_int32 * 3
    ws = lib.pda_dyn_voxel_workspace_bytes
    assert ws(i64(-1), 24) == -1 and ws(i64((1 << 30) + 1), 24) == -1 and ws(i64(1000), 0) == -1 and ws(i64(1000), 32) == -1
    assert ws(i64(0), 1) >= 0 and ws(i64(1000), 31) >= 4 * 4 * 1000 and ws(i64(180000 * 8), 28) > 0
    rng, vs = f6(-75.2, -75.2, -2, 75.2, 75.2, 4), f3(0.1, 0.1, 0.15)
    nul = [None] * 8

    def index(n, grid, batch, pillars):
        return lib.pda_dyn_voxel_index(None, i64(n), 6, rng, vs, i3(*grid), batch, pillars, *nul, None)

    # batch * cells >= 2^31: refused before any launch, whatever else is passed (the reference's int32 key would wrap)
    assert index(0, (1504, 1504, 40), 24, 0) == 1 and b"2^31" in lib.pda_last_error() and b"key range" in lib.pda_last_error()
    assert index(1000, (1504, 1504, 1000), 1, 0) == 1 and b"key range" in lib.pda_last_error()
    assert index(0, (46341, 46341, 1), 1, 1) == 1 and b"key range" in lib.pda_last_error()       # 46341^2 = 2^31 + 4633
    assert index(0, (46340, 46340, 40), 1, 1) == 0                                                # pillars: z takes no key bits
    assert index(0, (1504, 1504, 40), 23, 0) == 0                                                 # n == 0: OK, nothing touched
    assert index(1000, (1504, 1504, 40), 3, 0) == 1 and b"null" in lib.pda_last_error()
    assert index(0, (1504, 0, 40), 3, 0) == 1 and b"bad grid" in lib.pda_last_error()
    assert index(-1, (1504, 1504, 40), 3, 0) == 1 and index(0, (1504, 1504, 40), 0, 0) == 1 and index(0, (8, 8, 8), 1, 2) == 1
    assert lib.pda_dyn_scatter_mean(None, 0, None, None, None, i64(10), None, None) == 1
    assert lib.pda_dyn_scatter_mean(None, 3, None, None, None, i64(0), None, None) == 0
    assert lib.pda_dyn_scatter_max_fwd(None, 64, None, None, None, i64(10), None, None, None) == 1 and b"null" in lib.pda_last_error()
    assert lib.pda_dyn_scatter_max_bwd(None, None, None, None, i64(0), i64(0), 64, None, None) == 0
    assert lib.pda_dyn_pillar_features(None, i64(0), 3, *([None] * 5), vs, vs, 1, 0, None, None) == 1
    assert lib.pda_dyn_pillar_features(None, i64(0), 6, *([None] * 5), vs, vs, 1, 0, None, None) == 0


def test_python_layer_refuses_what_the_device_cannot_take(gold):
    from pdanet_amd import dyn_voxel_utils as dvu
    pts = torch.from_numpy(gold["points"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        dvu.dynamic_voxel_index(pts, _spec(gold, "voxel"), 3, pillars=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dvu.collate_packed(pts, torch.tensor([0, len(pts)]))
    with pytest.raises(ValueError, match="2\\^31"):
        dvu.dynamic_voxel_index(pts, _spec(gold, "voxel"), 24, pillars=False)
    assert dvu.pillar_feature_width(6, True, True) == 12 and dvu.pillar_feature_width(6, False, False) == 8


def test_generator_stand_in_loads(gold, generator):
    """The generator's stand-in torch_scatter: its contract on a case small enough to check by eye, and the fixture's
    stand-alone arrays recomputed by it.  The reference is not read."""
    assert "WAS NOT RUN" in generator.__doc__
    src = np.array([[1, 5], [3, 5], [3, 2], [0, 9], [3, 9]], np.float32)
    idx = np.array([1, 0, 1, 0, 1])
    out, arg = generator.scatter_max_np(src, idx, 2)
    assert out.tolist() == [[3, 9], [3, 9]] and arg.tolist() == [[1, 3], [2, 4]]          # ties: the first row stays
    mean = generator.scatter_mean_np(src, idx, 2)
    assert mean.dtype == np.float32 and mean.tolist() == [[1.5, 7.0], [np.float32(7) / np.float32(3), np.float32(16) / np.float32(3)]]
    had = sys.modules.get("torch_scatter")
    try:
        m = generator.install_torch_scatter()
        t = torch.from_numpy(src).requires_grad_(True)
        o, a = m.scatter_max(t, torch.from_numpy(idx), dim=0)
        (o * torch.tensor([[1.0, 2.0], [3.0, 4.0]])).sum().backward()
        assert a.tolist() == arg.tolist() and t.grad.tolist() == [[0, 0], [1, 0], [3, 0], [0, 2], [0, 4]]
    finally:
        sys.modules.pop("torch_scatter", None)
        if had is not None:
            sys.modules["torch_scatter"] = had
    inv, nv = gold["pillar_unq_inv"], len(gold["pillar_unq_cnt"])
    out, arg = generator.scatter_max_np(gold["smax_x"], inv, nv)
    assert np.array_equal(out, gold["smax_out"]) and np.array_equal(arg, gold["smax_arg"])
    xyz = gold["points"][gold["pillar_point_idx"]][:, 1:4]
    assert np.array_equal(_bits(generator.scatter_mean_np(xyz, inv, nv)), _bits(gold["pillar_mean"]))
    cnt = gold["voxel_unq_cnt"]
    assert cnt.max() > 1024 and (cnt == 257).any()
    assert (cnt == 1).sum() > 1000 and len(gold["pillar_point_idx"]) > len(gold["voxel_point_idx"])


# ---- on the device -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["voxel", "pillar"])
def test_index_matches_fixture(gold, setting):
    _, index = _run_index(gold, setting)
    got, want = _index_np(index), _expected(gold, setting)
    for k in want:      # whole padded arrays: the live part and the zeros beyond it
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    nk, nv = want["counts"]
    # the CSR lists every voxel's points in ascending order, each point once
    sp, ss, inv = got["seg_points"][:nk], got["seg_start"][:nv + 1], got["unq_inv"][:nk]
    assert ss[0] == 0 and ss[nv] == nk and np.array_equal(np.sort(sp), np.arange(nk))
    assert np.array_equal(inv[sp], np.repeat(np.arange(nv), np.diff(ss)))
    same = np.repeat(np.arange(nv), np.diff(ss))
    assert np.all((np.diff(sp) > 0) | (np.diff(same) > 0))


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["voxel", "pillar"])
def test_rows_the_reference_does_not_define_join_nothing(gold, setting):
    pts = gold["points"]
    nan = np.float32("nan")
    bad = pts[[5, 77, 1234, 3000, 4000, 5000]].copy()
    bad[0, 1] = nan                     # NaN x
    bad[1, 3] = nan                     # NaN z: joins nothing, pillars included
    bad[2, 0] = -1.0                    # batch index below the range
    bad[3, 0] = float(gold["batch"])    # ... and above it
    bad[4, 0] = nan
    bad[5, 2] = nan
    at = np.array([0, 300, 301, 2048, 4097, len(pts)])          # where they are inserted (positions in the original rows)
    mixed = np.insert(pts, at, bad, axis=0)
    keep = np.ones(len(mixed), bool)
    keep[at + np.arange(len(at))] = False
    new_row = np.nonzero(keep)[0]                               # original row -> row of `mixed`
    _, index = _run_index(gold, setting, mixed)
    got, want = _index_np(index), _expected(gold, setting)
    nk = want["counts"][0]
    assert np.array_equal(got["counts"], want["counts"])
    assert np.array_equal(got["point_idx"][:nk], new_row[want["point_idx"][:nk]]) and not got["point_idx"][nk:].any()
    for k in ("unq_inv", "unq_cnt", "voxel_coords", "seg_points", "seg_start"):
        m = len(want[k])
        assert np.array_equal(got[k][:m], want[k]) and not got[k][m:].any(), k


@pytest.mark.gpu
def test_scatter_mean_and_mean_vfe_bitwise(gold):
    from pdanet_amd import dyn_voxel_utils as dvu
    from pdanet_amd.dynamic_vfe import DynamicMeanVFE
    pts, index = _run_index(gold, "pillar")
    nv = len(gold["pillar_unq_cnt"])
    xyz = pts[:, 1:4][index.point_idx.long()].contiguous()
    mean = dvu.scatter_mean(xyz, index).cpu().numpy()
    assert mean.shape == (len(pts), 3) and np.array_equal(_bits(mean[:nv]), _bits(gold["pillar_mean"])) and not _bits(mean[nv:]).any()
    vfe = DynamicMeanVFE({}, 5, gold["voxel_size"].tolist(), gold["voxel_grid"].tolist(), gold["voxel_range"].tolist())
    assert vfe.get_output_feature_dim() == 5
    out = vfe({"points": pts, "batch_size": int(gold["batch"])})
    assert out["voxel_coords"].dtype == torch.int32 and np.array_equal(out["voxel_coords"].cpu().numpy(), gold["voxel_coords"])
    feats = out["voxel_features"].cpu().numpy()
    assert feats.shape == gold["voxel_features"].shape and np.array_equal(_bits(feats), _bits(gold["voxel_features"]))


@pytest.mark.gpu
@pytest.mark.parametrize("tag,use_abs,with_dist", CASES)
def test_pillar_features_bitwise(gold, tag, use_abs, with_dist):
    from pdanet_amd import dyn_voxel_utils as dvu
    pts, index = _run_index(gold, "pillar")
    mean = dvu.scatter_mean(pts[:, 1:4][index.point_idx.long()].contiguous(), index)
    feats = dvu.PillarFeatures.apply(pts, index, mean, _spec(gold, "pillar"), use_abs, with_dist).cpu().numpy()
    kept = gold["points"][gold["pillar_point_idx"]]
    fcols = gold["pillar_fcols"]
    want = np.concatenate([kept[:, 1:] if use_abs else kept[:, 4:], fcols if with_dist else fcols[:, :6]], 1)
    assert feats.shape == (len(pts), want.shape[1])
    assert np.array_equal(_bits(feats[:len(want)]), _bits(want)) and not _bits(feats[len(want):]).any()


@pytest.mark.gpu
def test_scatter_max_forward_and_backward(gold):
    from pdanet_amd import dyn_voxel_utils as dvu
    pts, index = _run_index(gold, "pillar")
    nk, nv = len(gold["pillar_unq_inv"]), len(gold["pillar_unq_cnt"])
    x = torch.from_numpy(gold["smax_x"]).cuda().requires_grad_(True)
    out, arg = dvu.ScatterMax.apply(x, index, nv)
    assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(gold["smax_out"]))
    assert arg.dtype == torch.int32 and np.array_equal(arg.cpu().numpy(), gold["smax_arg"])
    # padded form: rows beyond the voxel count are zero
    out_p, arg_p = dvu.ScatterMax.apply(x.detach(), index)
    assert out_p.shape == (len(pts), 8) and torch.equal(out_p[:nv], out.detach()) and not out_p[nv:].any() and not arg_p[nv:].any()
    # backward: grad_out[v, f] goes to row arg[v, f], everything else is zero
    go = np.random.default_rng(5).standard_normal((nv, 8)).astype(np.float32)
    want = np.zeros((nk, 8), np.float32)
    want[gold["smax_arg"], np.arange(8)[None, :]] = go
    (out * torch.from_numpy(go).cuda()).sum().backward()
    assert np.array_equal(_bits(x.grad.cpu().numpy()), _bits(want))
    # a buffer full of garbage comes back fully written: rows that are nobody's argmax are zero
    garbage = torch.full((nk, 8), float("nan"), device="cuda")
    got = dvu.scatter_max_backward(torch.from_numpy(go).cuda(), arg, index, nk, out=garbage).cpu().numpy()
    nobody = np.setdiff1d(np.arange(nk), gold["smax_arg"].reshape(-1))
    assert len(nobody) > 1000 and np.array_equal(_bits(got), _bits(want)) and not _bits(got[nobody]).any()


@pytest.mark.gpu
def test_two_runs_and_a_permutation_give_the_same_bits(gold, generator):
    from pdanet_amd import dyn_voxel_utils as dvu
    pts, a = _run_index(gold, "pillar")
    _, b = _run_index(gold, "pillar")
    ga, gb = _index_np(a), _index_np(b)
    assert all(np.array_equal(ga[k], gb[k]) for k in ga)
    xyz = pts[:, 1:4][a.point_idx.long()].contiguous()
    assert torch.equal(dvu.scatter_mean(xyz, a).view(torch.int32), dvu.scatter_mean(xyz, b).view(torch.int32))
    # the same rows in another order: the fixture's expectations re-derived by the permutation
    n = len(gold["points"])
    perm = np.random.default_rng(9).permutation(n)              # row j of the permuted input is row perm[j] of the fixture's
    where = np.empty(n, np.int64)
    where[perm] = np.arange(n)
    for setting in ("voxel", "pillar"):
        want = _expected(gold, setting)
        nk, nv = want["counts"]
        _, index = _run_index(gold, setting, gold["points"][perm])
        got = _index_np(index)
        for k in ("counts", "unq_cnt", "voxel_coords", "seg_start"):          # per voxel: identical
            assert np.array_equal(got[k], want[k]), (setting, k)
        new_idx = np.sort(where[want["point_idx"][:nk]])                       # per point: permuted
        assert np.array_equal(got["point_idx"][:nk], new_idx) and not got["point_idx"][nk:].any()
        old_pos = np.empty(n, np.int64)
        old_pos[want["point_idx"][:nk]] = np.arange(nk)                        # fixture row -> its kept position
        pos = old_pos[perm[new_idx]]                                           # new kept position -> fixture's kept position
        assert np.array_equal(got["unq_inv"][:nk], want["unq_inv"][:nk][pos]) and not got["unq_inv"][nk:].any()
        assert np.array_equal(got["seg_points"][:nk], np.argsort(got["unq_inv"][:nk], kind="stable"))
        if setting == "pillar":
            x = gold["smax_x"][pos]
            out, arg = dvu.ScatterMax.apply(torch.from_numpy(x).cuda(), index, nv)
            w_out, w_arg = generator.scatter_max_np(x, got["unq_inv"][:nk], nv)
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(gold["smax_out"])) and np.array_equal(w_out, gold["smax_out"])
            assert np.array_equal(arg.cpu().numpy(), w_arg)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,use_abs,with_dist", CASES)
def test_dynamic_pillar_vfe_train_mode(gold, tag, use_abs, with_dist):
    """pillar_features and the gradients against the reference module run in float64; allowed: 4 x the deviation of the
    reference's own float32 CPU run from that float64 run (dev_ref_*)."""
    vfe = _pillar_vfe(gold, use_abs, with_dist)
    state = {k: torch.from_numpy(gold["%s_state.%s" % (tag, k)]) for k in gold[tag + "_state_keys"].tolist()}
    vfe.load_state_dict(state, strict=True)                    # a reference-shaped checkpoint
    vfe = vfe.cuda().train()
    pts = torch.from_numpy(gold["points"]).cuda().requires_grad_(True)
    out = vfe({"points": pts, "batch_size": int(gold["batch"])})
    pf = out["pillar_features"]
    assert out["voxel_coords"].dtype == torch.int32 and np.array_equal(out["voxel_coords"].cpu().numpy(), gold["pillar_coords"])
    v, f = np.meshgrid(np.arange(pf.shape[0]), np.arange(pf.shape[1]), indexing="ij")
    proj = torch.from_numpy(np.sin(0.37 * v + 1.3 * f + 0.5)).to(torch.float32).cuda()
    (pf.sum() + (pf * proj).sum()).backward()
    got = {"pillar_features": pf.detach(), "grad_extra": pts.grad[:, 4:]}
    for k, p in vfe.named_parameters():
        got["grad." + k] = p.grad
    assert not pts.grad[:, :4].any()                           # the coordinates are inputs
    worst = []
    for k, t in got.items():
        want, allowed = _f64(gold, "%s_%s" % (tag, k)), 4.0 * float(gold["dev_ref_%s_%s" % (tag, k)])
        dev = float(np.abs(t.cpu().numpy().astype(np.float64) - want).max())
        print("%s %s: deviation %.3g, allowed %.3g" % (tag, k, dev, allowed))
        assert t.shape == want.shape
        if not dev <= allowed:
            worst.append((k, dev, allowed))
    assert not worst, worst


@pytest.mark.gpu
def test_collate_packed():
    from pdanet_amd.dyn_voxel_utils import collate_packed
    rng = np.random.default_rng(3)
    sizes = [5, 0, 300, 1, 0]                                   # empty scenes in the middle and at the end
    pts = rng.standard_normal((sum(sizes), 4)).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    want = np.concatenate([np.concatenate([np.full((s, 1), b, np.float32), pts[offs[b]:offs[b + 1]]], 1) for b, s in enumerate(sizes)])
    got = collate_packed(torch.from_numpy(pts).cuda(), torch.from_numpy(offs).cuda())
    assert got.dtype == torch.float32 and np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    none = collate_packed(torch.zeros((0, 4)).cuda(), torch.zeros((3,), dtype=torch.int64).cuda())
    assert none.shape == (0, 5)
