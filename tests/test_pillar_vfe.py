"""The hard-voxel PillarVFE (pdanet_amd/pillar_vfe.py, pda_pillar_features) and voxel_utils.collate_voxels against
tests/golden/anchor_head.npz, the reference's PillarVFE on CPU tensors (tests/golden/make_anchor_head_golden.py): 203 voxels
of 32 rows and 4 columns, among them voxels with 1 and with 32 points, with (USE_ABSLOTE_XYZ True, WITH_DISTANCE False) and
(False, True).

Tolerances.  Raw and centre columns are copies and single float32 operations: bit-identical; padded rows exactly 0.  The
xyz - mean columns stay within 64 * 2^-24 * max|coordinate of that voxel|: two summation orders of at most 32 float32 terms
can differ by twice (n - 1) u max|x|.  The distance column is three squares, two additions and a square root on both
sides, possibly added in another order: 2 ulp.  The module's output within 2e-5 of the fixture (absolute; the values are of
order one)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from pdanet_amd import _lib
from pdanet_amd.config import to_attr
from pdanet_amd.pillar_vfe import PFNLayer, PillarVFE, pillar_features  # noqa: F401
from pdanet_amd.voxel_utils import collate_voxels

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import anchor_head_restatement as rs  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "anchor_head.npz"))
CFG = json.loads(str(G['configs']))['a']
PCR, VS = CFG['point_cloud_range'], CFG['voxel_size']
CASES = ['p', 'q']


def ulps(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)

    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(a) - ordered(b))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def model_cfg(tag):
    return json.loads(str(G['v%s_cfg' % tag]))


def check_features(tag, got):
    cfg = model_cfg(tag)
    ref, vox, num = G['v%s_features' % tag], G['v_voxels'], G['v_num_points']
    assert got.shape == ref.shape and got.dtype == np.float32
    raw = 4 if cfg['USE_ABSLOTE_XYZ'] else 1
    pad = np.arange(vox.shape[1])[None, :] >= num[:, None]
    assert not got[pad].any(), "padded rows"
    live = ~pad                      # the reference's padded rows are x * 0 and carry the sign of x: zero, not the bits of +0
    assert not ref[pad].any()
    assert bits_equal(got[live][:, :raw], ref[live][:, :raw]), "raw columns"
    assert bits_equal(got[live][:, raw + 3:raw + 6], ref[live][:, raw + 3:raw + 6]), "centre columns"
    bound = 64 * 2.0 ** -24 * np.abs(vox[..., :3]).max(axis=(1, 2))
    d = np.abs(got[..., raw:raw + 3].astype(np.float64) - ref[..., raw:raw + 3]).max(axis=(1, 2))
    print("features", tag, "largest mean-column difference over its bound: %.3g" % float((d / bound).max()))
    assert (d <= bound).all(), "xyz - mean columns"
    if cfg['WITH_DISTANCE']:
        assert ulps(got[..., -1], ref[..., -1]).max() <= 2, "distance column"


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_symbol_and_fixture():
    assert "pda_pillar_features" in _lib.SIGNATURES
    num = G['v_num_points']
    assert G['v_voxels'].shape == (203, 32, 4) and num[0] == 1 and num[1] == 32 and 1 <= num.min() and num.max() == 32
    assert [model_cfg(t)['USE_ABSLOTE_XYZ'] for t in CASES] == [True, False] and model_cfg('q')['WITH_DISTANCE']


@pytest.mark.parametrize("tag", CASES)
def test_restatement_features(tag):
    cfg = model_cfg(tag)
    check_features(tag, rs.pillar_features(G['v_voxels'], G['v_num_points'], G['v_coords'], VS, PCR, cfg['USE_ABSLOTE_XYZ'],
                                           cfg['WITH_DISTANCE']))


@pytest.mark.parametrize("tag", CASES)
def test_state_dict_keys_are_the_references(tag):
    vfe = PillarVFE(to_attr(model_cfg(tag)), num_point_features=4, voxel_size=VS, point_cloud_range=PCR)
    assert list(vfe.state_dict().keys()) == [str(k) for k in G['v%s_keys' % tag]]
    assert vfe.get_output_feature_dim() == 16
    vfe.load_state_dict({str(k): torch.from_numpy(G['v%s_sd_%s' % (tag, k)]) for k in G['v%s_keys' % tag]}, strict=True)


def test_no_cpu_path_and_no_backward():
    vox, num, crd = torch.from_numpy(G['v_voxels']), torch.from_numpy(G['v_num_points']), torch.from_numpy(G['v_coords'])
    with pytest.raises(RuntimeError, match="no CPU path"):
        pillar_features(vox, num, crd, VS, PCR)
    vfe = PillarVFE(to_attr(model_cfg('p')), num_point_features=4, voxel_size=VS, point_cloud_range=PCR)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vfe({'voxels': vox, 'voxel_num_points': num, 'voxel_coords': crd})
    with pytest.raises(RuntimeError, match="no backward"):
        pillar_features(vox.clone().requires_grad_(True), num, crd, VS, PCR)
    with pytest.raises(ValueError):
        pillar_features(vox[..., :2], num, crd, VS, PCR)


def test_argument_validation_without_gpu():
    import ctypes
    lib = _lib.load()
    f3 = (ctypes.c_float * 3)(0.2, 0.2, 4.0)
    call = lambda v, p, c: lib.pda_pillar_features(None, None, None, ctypes.c_int64(v), p, c, f3, f3, 1, 0, None, None)
    assert call(-1, 32, 4) == 1 and call(8, 32, 2) == 1 and b"c=2" in lib.pda_last_error()
    assert call(0, 32, 4) == 0 and call(8, 0, 4) == 0
    assert call(8, 32, 4) == 1 and b"null" in lib.pda_last_error()


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@gpu
@pytest.mark.parametrize("tag", CASES)
def test_gpu_features(tag):
    cfg = model_cfg(tag)
    got = pillar_features(dev(G['v_voxels']), dev(G['v_num_points']), dev(G['v_coords']), VS, PCR, cfg['USE_ABSLOTE_XYZ'],
                          cfg['WITH_DISTANCE'])
    check_features(tag, got.cpu().numpy())
    # int64 counts and coordinates, as a collate function of the reference hands them over
    again = pillar_features(dev(G['v_voxels']), dev(G['v_num_points']).long(), dev(G['v_coords']).long(), VS, PCR,
                            cfg['USE_ABSLOTE_XYZ'], cfg['WITH_DISTANCE'])
    assert torch.equal(got, again)


@gpu
@pytest.mark.parametrize("tag", CASES)
def test_gpu_module_output(tag):
    vfe = PillarVFE(to_attr(model_cfg(tag)), num_point_features=4, voxel_size=np.array(VS), point_cloud_range=np.array(PCR))
    vfe.load_state_dict({str(k): torch.from_numpy(G['v%s_sd_%s' % (tag, k)]) for k in G['v%s_keys' % tag]}, strict=True)
    vfe = vfe.cuda()
    batch = lambda: {'voxels': dev(G['v_voxels']), 'voxel_num_points': dev(G['v_num_points']), 'voxel_coords': dev(G['v_coords'])}
    for mode in ('eval', 'train'):
        getattr(vfe, mode)()
        out = vfe(batch())['pillar_features']
        ref = G['v%s_out_%s' % (tag, mode)]
        assert out.shape == ref.shape
        d = float(np.abs(out.detach().cpu().numpy().astype(np.float64) - ref).max())
        print("module", tag, mode, "%.3g" % d)
        assert d <= 2e-5
    out.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in vfe.parameters())


@gpu
def test_gpu_collate_voxels():
    B, cap, P, C = 3, 6, 4, 4
    rng = np.random.default_rng(3)
    voxels, coords = rng.random((B, cap, P, C)).astype(np.float32), rng.integers(0, 9, (B, cap, 3)).astype(np.int32)
    num_points = rng.integers(1, P + 1, (B, cap)).astype(np.int32)
    num_voxels = np.array([4, 0, 6], np.int32)
    v, c, n = collate_voxels(dev(voxels), dev(coords), dev(num_points), dev(num_voxels))
    assert v.shape == (10, P, C) and c.shape == (10, 4) and n.shape == (10,) and c.dtype == torch.int32
    assert np.array_equal(c[:, 0].cpu().numpy(), [0] * 4 + [2] * 6)
    assert bits_equal(v.cpu().numpy(), np.concatenate([voxels[0, :4], voxels[2]])) and v.is_contiguous()
    assert np.array_equal(c[:, 1:].cpu().numpy(), np.concatenate([coords[0, :4], coords[2]]))
    assert np.array_equal(n.cpu().numpy(), np.concatenate([num_points[0, :4], num_points[2]]))
