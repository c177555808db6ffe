"""RoI pooling of the two-stage heads: roiaware_pool3d forward / backward, roipoint_pool3d forward and the device form of
points_in_boxes_cpu (include/pda_train.h, csrc/roi_pool.hip).

CPU: the boundary (names, exported symbols, argument validation, no CPU path), hand-derived known answers of the numpy
restatement of the reference's kernels (tests/golden/roi_pool_restatement.py) and the restatement against the reference's
own Python composition (tests/golden/roi_pool.npz).
GPU: HIP == restatement, index-exact and bitwise for both forwards; the max backward exactly (integer gradients), the avg
backward within a bound derived per element; the reference's composition through roi_pool.npz; the uncontracted build.

Inputs: tests/golden/roi_pool_inputs.py.  The generic roiaware generator drops 2.1 % of the in-box (point, box) pairs
(cap 5 %, asserted there and in test_generic_inputs_keep_their_cap)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import roi_pool_inputs as gen  # noqa: E402
import roi_pool_restatement as ref  # noqa: E402

I32, F32, F64 = np.int32, np.float32, np.float64
U = 2.0 ** -24                                   # unit roundoff of float32

AWARE_CUDA_NAMES = ["forward", "backward", "points_in_boxes_gpu", "points_in_boxes_cpu"]
AWARE_NAMES = ["RoIAwarePool3d", "RoIAwarePool3dFunction", "points_in_boxes_cpu", "points_in_boxes_gpu"]
POINT_NAMES = ["RoIPointPool3d", "RoIPointPool3dFunction"]
SYMBOLS = ["pda_roiaware_pool3d_fwd", "pda_roiaware_pool3d_bwd", "pda_roipoint_pool3d_fwd", "pda_points_in_boxes_mask"]

OUT_SIZES = [(3, 4, 5), 12, (40, 40, 8)]          # 12^3 = 1728 voxels: counters in LDS; 40 * 40 * 8 = 12800: counters in place
K_SLOTS = [4, 128]                                # 4: the cap is hit and the cluster's count reads 3
METHODS = ["max", "avg"]


def _grid(out_size):
    return (out_size,) * 3 if isinstance(out_size, int) else tuple(out_size)


@pytest.fixture(scope="module")
def lib():
    from pdanet_amd import build, _lib
    build.build()
    return _lib.load()


# ---------------------------------------------------------------- the boundary (no GPU) ----------------------------
def test_reference_names_exist():
    from pdanet_amd import roiaware_pool3d_utils as au, roipoint_pool3d_utils as pu
    for name in AWARE_CUDA_NAMES:
        assert callable(getattr(au.roiaware_pool3d_cuda, name)), name
    for name in AWARE_NAMES:
        assert callable(getattr(au, name)), name
    assert callable(pu.roipoint_pool3d_cuda.forward)
    for name in POINT_NAMES:
        assert callable(getattr(pu, name)), name
    pool = pu.RoIPointPool3d()
    assert pool.num_sampled_points == 512 and pool.pool_extra_width == 1.0
    assert au.RoIAwarePool3d(7).max_pts_each_voxel == 128


def test_symbols_exported(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), "libpda_pointnet2.so does not export %s" % name
    assert lib.pda_abi_version() == 20


def test_bad_sizes_and_empty_problems(lib):
    N = None
    err = lambda: lib.pda_last_error()  # noqa: E731
    # fwd: (rois, pts, feat, argmax, slots, pooled, boxes, points, channels, K, ox, oy, oz, method, stream)
    fwd = lambda n, p, c, k, ox, oy, oz, m=0: lib.pda_roiaware_pool3d_fwd(N, N, N, N, N, N, n, p, c, k, ox, oy, oz, m, N)  # noqa: E731
    assert fwd(4, 8, 3, 8, 256, 4, 4) == 1 and b"pda_roiaware_pool3d_fwd" in err()
    assert fwd(4, 8, 3, 8, 4, 4, 0) == 1 and fwd(4, 8, 3, 8, 4, 256, 4) == 1
    assert fwd(4, 8, 3, 0, 4, 4, 4) == 1 and b"pda_roiaware_pool3d_fwd" in err()
    assert fwd(-1, 8, 3, 8, 4, 4, 4) == 1 and fwd(4, -8, 3, 8, 4, 4, 4) == 1 and fwd(4, 8, -3, 8, 4, 4, 4) == 1
    assert fwd(4, 8, 3, 8, 4, 4, 4, 2) == 1 and b"pool_method" in err()
    assert fwd(4, 8, 3, 8, 4, 4, 4) == 1 and b"pda_roiaware_pool3d_fwd: null" in err()
    assert fwd(0, 8, 3, 8, 4, 4, 4) == 0 and fwd(4, 0, 3, 8, 255, 255, 255, 1) == 0
    # bwd: (slots, argmax, grad_out, grad_in, boxes, points, channels, K, ox, oy, oz, method, stream)
    bwd = lambda n, p, c, k, ox, oy, oz, m=0: lib.pda_roiaware_pool3d_bwd(N, N, N, N, n, p, c, k, ox, oy, oz, m, N)  # noqa: E731
    assert bwd(4, 8, 3, 8, 4, 4, 256) == 1 and b"pda_roiaware_pool3d_bwd" in err()
    assert bwd(4, 8, 3, 0, 4, 4, 4) == 1 and bwd(-4, 8, 3, 8, 4, 4, 4) == 1 and bwd(4, 8, 3, 8, 4, 4, 4, -1) == 1
    assert bwd(4, 8, 3, 8, 4, 4, 4, 1) == 1 and b"pda_roiaware_pool3d_bwd: null" in err()
    assert bwd(0, 8, 3, 8, 4, 4, 4) == 0 and bwd(4, 0, 3, 8, 4, 4, 4, 1) == 0
    # roipoint: (xyz, boxes, feat, pooled, flag, batch, points, boxes, channels, sampled, stream)
    rpp = lambda b, p, m, c, s: lib.pda_roipoint_pool3d_fwd(N, N, N, N, N, b, p, m, c, s, N)  # noqa: E731
    assert rpp(2, 8, 4, 3, 0) == 1 and b"pda_roipoint_pool3d_fwd" in err()
    assert rpp(-2, 8, 4, 3, 16) == 1 and rpp(2, -8, 4, 3, 16) == 1 and rpp(2, 8, -4, 3, 16) == 1
    assert rpp(2, 8, 4, 3, 1 << 20) == 1 and b"LDS" in err()       # an S that does not fit is refused
    assert rpp(70000, 8, 4, 3, 16) == 1 and b"65535" in err()
    assert rpp(2, 8, 4, 3, 512) == 1 and b"pda_roipoint_pool3d_fwd: null" in err()
    assert rpp(0, 8, 4, 3, 16) == 0 and rpp(2, 0, 4, 3, 16) == 0 and rpp(2, 8, 0, 3, 16) == 0
    # mask: (boxes, pts, mask, boxes, points, stream)
    assert lib.pda_points_in_boxes_mask(N, N, N, -1, 8, N) == 1 and b"pda_points_in_boxes_mask" in err()
    assert lib.pda_points_in_boxes_mask(N, N, N, 4, 8, N) == 1 and b"pda_points_in_boxes_mask: null" in err()
    assert lib.pda_points_in_boxes_mask(N, N, N, 0, 8, N) == 0 and lib.pda_points_in_boxes_mask(N, N, N, 4, 0, N) == 0


def test_ops_refuse_cpu_tensors():
    import torch
    from pdanet_amd import roiaware_pool3d_utils as au, roipoint_pool3d_utils as pu
    rois, pts, feat = torch.zeros(2, 7), torch.zeros(8, 3), torch.zeros(8, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        au.RoIAwarePool3d(3, 4)(rois, pts, feat)
    with pytest.raises(RuntimeError, match="no CPU path"):
        au.roiaware_pool3d_cuda.backward(torch.zeros(2, 3, 3, 3, 4, dtype=torch.int32), torch.zeros(2, 3, 3, 3, 4, dtype=torch.int32),
                                         torch.zeros(2, 3, 3, 3, 4), torch.zeros(8, 4), 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        au.roiaware_pool3d_cuda.points_in_boxes_cpu(rois, pts, torch.zeros(2, 8, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        pu.RoIPointPool3d(16, 1.0)(torch.zeros(1, 8, 3), torch.zeros(1, 8, 4), torch.zeros(1, 2, 7))


# ---------------------------------------------------------------- known answers of the restatement -----------------
# one box (centre 0, size 2 x 2 x 2, heading 0), grid (2, 2, 1): voxel x index 0 for local x < 0, 1 from 0 on; every
# point has y = 0 and (0 + 1) / 1 = 1 puts it in y index 1, so the voxels (x, 0, 0) stay empty
_KA_BOX = np.array([[0, 0, 0, 2, 2, 2, 0]], F32)
_KA_PTS = np.array([[-0.5, 0, 0],     # 0: voxel x0
                    [0.5, 0, 0],      # 1: voxel x1
                    [-0.25, 0, 0],    # 2: voxel x0, its second point
                    [-0.75, 0, 0],    # 3: voxel x0, its third point: dropped with K = 3 (two slots)
                    [5, 0, 0],        # 4: outside
                    [1.0, 0, 0],      # 5: ON the face: |x| < 1 + 1e-5 is inside; (1 + 1) / 1 = 2 is clamped to x1
                    [0, 0, 0]],       # 6: ON the voxel boundary: (0 + 1) / 1 = 1 -> x1, its third point: dropped
                   F32)
_KA_FEAT = np.array([[1, 5], [2, 2], [1, 7], [9, 9], [8, 8], [2, 4], [6, 6]], F32)


def _ka_aware(method, k_slots=3, feat=_KA_FEAT):
    am, sl = np.zeros((1, 2, 2, 1, 2), I32), np.zeros((1, 2, 2, 1, k_slots), I32)
    pf = np.full((1, 2, 2, 1, 2), 7, F32)                           # a sentinel: what "untouched" leaves
    runs = []
    for contract in (0, 1):
        am2, sl2, pf2 = am.copy(), sl.copy(), pf.copy()
        ref.roiaware_pool3d_forward(_KA_BOX, _KA_PTS, feat, am2, sl2, pf2, method, contract)
        runs.append((am2[0, :, :, 0], sl2[0, :, :, 0], pf2[0, :, :, 0]))
    assert all(np.array_equal(x, y) for x, y in zip(*runs))          # heading 0 on a lattice: either contraction mode
    return runs[0]


def test_restatement_slot_order_cap_tie_and_empty_voxel():
    am, sl, pf = _ka_aware(0)
    # slot 0 = count capped at K - 1 = 2; then the first two points of the voxel in ascending index
    assert sl[0, 1].tolist() == [2, 0, 2] and sl[1, 1].tolist() == [2, 1, 5]
    assert sl[0, 0].tolist() == [0, 0, 0] and sl[1, 0].tolist() == [0, 0, 0]
    # max, voxel x0: channel 0 is 1 (point 0) against 1 (point 2): strict > keeps the lower slot; channel 1: 5 < 7
    assert am[0, 1].tolist() == [0, 2] and pf[0, 1].tolist() == [1, 7]
    # voxel x1: channel 0 is 2 (point 1) against 2 (point 5): point 1; channel 1: 2 < 4: point 5.  Points 3 and 6 (9 and 6) were dropped
    assert am[1, 1].tolist() == [1, 5] and pf[1, 1].tolist() == [2, 4]
    # empty voxels: argmax -1, pooled_features untouched
    assert am[0, 0].tolist() == [-1, -1] and am[1, 0].tolist() == [-1, -1] and pf[0, 0].tolist() == [7, 7] and pf[1, 0].tolist() == [7, 7]
    # with room for everything (K = 8) the dropped points come back, in index order
    am, sl, pf = _ka_aware(0, 8)
    assert sl[0, 1].tolist() == [3, 0, 2, 3, 0, 0, 0, 0] and sl[1, 1].tolist() == [3, 1, 5, 6, 0, 0, 0, 0]
    assert am[0, 1].tolist() == [3, 3] and pf[1, 1].tolist() == [6, 6]
    # K = 1: no slot at all, every count stays 0
    am, sl, pf = _ka_aware(0, 1)
    assert not sl.any() and (am == -1).all() and (pf == 7).all()


def test_restatement_nan_and_minus_inf_never_win():
    feat = _KA_FEAT.copy()
    feat[0] = [np.nan, -np.inf]
    feat[2] = [-3, -np.inf]
    am, sl, pf = _ka_aware(0, feat=feat)
    # voxel x0 holds points 0 and 2: channel 0 NaN > -inf is false, -3 wins; channel 1 is -inf twice: nothing wins, untouched
    assert am[0, 1].tolist() == [2, -1] and pf[0, 1].tolist() == [-3, 7]


def test_restatement_avg_of_one_two_and_three_points():
    box = np.array([[0, 0, 0, 3, 2, 2, 0]], F32)                    # grid (3, 1, 1): voxels of width 1 along x
    pts = np.array([[-1, 0, 0], [0, 0, 0], [0.25, 0, 0], [1, 0, 0], [1.25, 0, 0], [1.4, 0, 0]], F32)
    a, b, c = F32(0.1), F32(0.2), F32(0.3)
    feat = np.array([[a], [a], [b], [a], [b], [c]], F32)
    am, sl, pf = np.zeros((1, 3, 1, 1, 1), I32), np.zeros((1, 3, 1, 1, 5), I32), np.zeros((1, 3, 1, 1, 1), F32)
    ref.roiaware_pool3d_forward(box, pts, feat, am, sl, pf, 1)
    assert sl[0, :, 0, 0, 0].tolist() == [1, 2, 3] and not am.any()     # avg leaves argmax alone
    # a sequential float32 sum in slot order, divided once by float(count)
    assert pf[0, 0, 0, 0, 0] == F32(a / F32(1))
    assert pf[0, 1, 0, 0, 0] == F32(F32(a + b) / F32(2))
    assert pf[0, 2, 0, 0, 0] == F32(F32(F32(a + b) + c) / F32(3))
    # backward, avg: grad 1 into the three voxels -> 1, 1/2, 1/2, 1/3, 1/3, 1/3; max: the argmax only
    s, mag, n = ref.roiaware_pool3d_backward_terms(sl, am, np.ones((1, 3, 1, 1, 1), F32), 6, 1)
    assert np.allclose(s[:, 0], [1, .5, .5, 1 / 3, 1 / 3, 1 / 3], rtol=1e-15) and n[:, 0].tolist() == [1] * 6
    am[:] = [[[[[-1]]], [[[2]]], [[[2]]]]]
    s, mag, n = ref.roiaware_pool3d_backward_terms(sl, am, np.full((1, 3, 1, 1, 1), 3, F32), 6, 0)
    assert s[:, 0].tolist() == [0, 0, 6, 0, 0, 0] and n[:, 0].tolist() == [0, 0, 2, 0, 0, 0] and mag[2, 0] == 6


def test_restatement_voxel_index_keeps_the_unsigned_clamp():
    # d = 1, four voxels of width 0.25: local -0.6 -> (-0.6 + 0.5) / 0.25 = -0.4 truncates to 0; local -0.8 -> -1.2 truncates
    # to -1, which as an unsigned value is clamped to the LAST voxel (only reachable where a voxel is thinner than the margin)
    assert ref.voxel_axis(F32(-0.6), F32(1), 4) == 0 and ref.voxel_axis(F32(-0.8), F32(1), 4) == 3
    assert ref.voxel_axis(F32(0.5), F32(1), 4) == 3 and ref.voxel_axis(F32(0.25), F32(1), 4) == 3 and ref.voxel_axis(F32(0.2), F32(1), 4) == 2


def test_restatement_roipoint_wrap_and_empty_flag():
    xyz = np.array([[[5, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [0, 0, 5], [0, 0, -1]]], F32)   # 1, 2 and 4 inside (z on the face)
    boxes = np.array([[[0, 0, 0, 2, 2, 2, 0], [20, 0, 0, 2, 2, 2, 0]]], F32)
    feat = np.arange(10, dtype=F32).reshape(1, 5, 2)
    rows, flag = np.full((1, 2, 7, 5), 9, F32), np.zeros((1, 2), I32)
    ref.roipoint_pool3d_forward(xyz, boxes, feat, rows, flag)
    # cnt = 3 < S = 7: slots 3.. repeat slot k % 3
    assert rows[0, 0, :, 3].tolist() == [2, 4, 8, 2, 4, 8, 2] and rows[0, 0, 2].tolist() == [0, 0, -1, 8, 9]
    assert flag.tolist() == [[0, 1]] and (rows[0, 1] == 9).all()        # the empty box: flag 1, rows untouched
    rows, flag = np.zeros((1, 2, 2, 5), F32), np.zeros((1, 2), I32)
    ref.roipoint_pool3d_forward(xyz, boxes, feat, rows, flag)
    assert rows[0, 0, :, 3].tolist() == [2, 4]                          # cnt > S: the first S in ascending index


def test_restatement_margins_of_the_device_and_the_host_test():
    box = np.array([[0, 0, 0, 2, 2, 2, 0]], F32)
    pts = np.array([[1.005, 0, 0], [0, 1.0000001, 0], [0, 0, 1.005]], F32)     # 5e-3 outside the x face; inside; outside in z
    mask = np.zeros((1, 3), I32)
    ref.points_in_boxes_cpu(box, pts, mask)
    assert mask.tolist() == [[1, 1, 0]]                                 # margin 1e-2 on x and y, none on z
    assert ref.in_box(pts, box[0], ref.MARGIN_GPU, 1)[0].tolist() == [False, True, False]   # margin 1e-5


def test_generic_inputs_keep_their_cap():
    a = gen.roiaware_inputs("generic")
    assert 0 < a["drop"] <= 0.05
    print("generic roiaware inputs: %.2f %% of the in-box pairs dropped" % (100 * a["drop"]))
    for kind in ("exact", "generic"):
        inp = gen.roiaware_inputs(kind)
        hits = np.stack([ref.in_box(inp["pts"], r, ref.MARGIN_GPU, 1)[0] for r in inp["rois"]])
        assert hits[0].sum() == 0 and (hits[1] & hits[2]).sum() >= 5 and hits[4][gen.CLUSTER].all() and hits[5].sum() > 20
        b = gen.roipoint_inputs(kind)
        assert b["counts"].tolist() == [[512, 16, 20, 540, 0], [512, 7, 20, 540, 0]] and b["counts_wide"][0, 4] == 3


# ---------------------------------------------------------------- restatement == the reference's composition -------
@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(HERE, "golden", "roi_pool.npz"))


def _bits(a):
    return np.ascontiguousarray(a).view(I32)


def test_restatement_reproduces_the_golden_file():
    z = _golden()
    for contract in (0, 1):                                            # lattice inputs: either mode
        for tag in [str(t) for t in z["aware_cases"]]:
            ox, oy, oz, k, method = (int(v) for v in z[tag + "_args"])
            am, sl = np.zeros((6, ox, oy, oz, 3), I32), np.zeros((6, ox, oy, oz, k), I32)
            pf = np.zeros((6, ox, oy, oz, 3), F32)
            ref.roiaware_pool3d_forward(z["rois"], z["pts"], z["feat"], am, sl, pf, method, contract)
            assert np.array_equal(sl, z[tag + "_slots"]) and np.array_equal(am, z[tag + "_argmax"])
            assert np.array_equal(_bits(pf), _bits(z[tag + "_out"]))
            gi = np.zeros((gen.P, 3), F32)
            ref.roiaware_pool3d_backward(sl, am, z[tag + "_grad_out"], gi, method)
            assert np.array_equal(_bits(gi), _bits(z[tag + "_grad_in"]))
        for tag in [str(t) for t in z["point_cases"]]:
            s, w = int(z[tag + "_args"][0]), F32(z[tag + "_args"][1])
            boxes = z["boxes"].copy()
            boxes[..., 3:6] += w
            rows, flag = np.zeros((2, 5, s, 8), F32), np.zeros((2, 5), I32)
            ref.roipoint_pool3d_forward(z["xyz"], boxes, z["pfeat"], rows, flag, contract)
            assert np.array_equal(_bits(rows), _bits(z[tag + "_rows"])) and np.array_equal(flag, z[tag + "_flag"])
    mask = np.zeros((6, gen.P), I32)
    ref.points_in_boxes_cpu(z["rois"], z["pts"], mask)
    assert np.array_equal(mask, z["mask"]) and mask.sum() > 100


# ---------------------------------------------------------------- GPU helpers ---------------------------------------
@functools.lru_cache(maxsize=None)
def _contract():
    from pdanet_amd import _lib
    return int(_lib.load().pda_fp_contract_mode())


@functools.lru_cache(maxsize=None)
def _aware_inputs(kind):
    return gen.roiaware_inputs(kind)


@functools.lru_cache(maxsize=None)
def _point_inputs(kind):
    return gen.roipoint_inputs(kind)


@functools.lru_cache(maxsize=2)
def _ref_collect(kind, grid, k_slots):
    """slots of the restatement (they do not depend on the features or the method)"""
    inp = _aware_inputs(kind)
    sl = np.zeros((6,) + grid + (k_slots,), I32)
    ref.roiaware_pool3d_forward(inp["rois"], inp["pts"], np.zeros((gen.P, 0), F32), np.zeros((6,) + grid + (0,), I32), sl,
                                np.zeros((6,) + grid + (0,), F32), 1, _contract())
    sl.setflags(write=False)
    return sl


@functools.lru_cache(maxsize=2)
def _ref_aware(kind, c, grid, k_slots, method):
    inp = _aware_inputs(kind)
    am, sl = np.zeros((6,) + grid + (c,), I32), np.zeros((6,) + grid + (k_slots,), I32)
    pf = np.zeros((6,) + grid + (c,), F32)
    ref.roiaware_pool3d_forward(inp["rois"], inp["pts"], inp["feat%d" % c], am, sl, pf, method, _contract())
    for a in (am, sl, pf):
        a.setflags(write=False)
    return am, sl, pf


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: cached references are read-only


def _gpu_aware(inp, c, grid, k_slots, method):
    import torch
    from pdanet_amd import roiaware_pool3d_utils as au
    am = torch.zeros((6,) + grid + (c,), dtype=torch.int32, device="cuda")
    sl = torch.zeros((6,) + grid + (k_slots,), dtype=torch.int32, device="cuda")
    pf = torch.zeros((6,) + grid + (c,), device="cuda")
    assert au.roiaware_pool3d_cuda.forward(_t(inp["rois"]), _t(inp["pts"]), _t(inp["feat%d" % c]), am, sl, pf, method) == 1
    return am.cpu().numpy(), sl.cpu().numpy(), pf.cpu().numpy()


# ---------------------------------------------------------------- HIP == restatement -------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("k_slots", K_SLOTS)
@pytest.mark.parametrize("out_size", OUT_SIZES, ids=str)
@pytest.mark.parametrize("c", [3, 70])
@pytest.mark.parametrize("kind", ["exact", "generic"])
def test_hip_roiaware_forward(kind, c, out_size, k_slots, method):
    grid, m = _grid(out_size), METHODS.index(method)
    w_am, w_sl, w_pf = _ref_aware(kind, c, grid, k_slots, m)
    am, sl, pf = _gpu_aware(_aware_inputs(kind), c, grid, k_slots, m)
    assert np.array_equal(sl, w_sl)
    assert np.array_equal(am, w_am)
    assert np.array_equal(_bits(pf), _bits(w_pf))
    # the inputs do what they are there for: an empty box, voxels shared by two boxes' points, the cluster at the cap
    cnt = w_sl[..., 0].reshape(6, -1)
    assert cnt[0].sum() == 0 and cnt.max() == (3 if k_slots == 4 else 9) and (cnt > 0).sum() > 100
    cluster = w_sl[4].reshape(-1, k_slots)[cnt[4].argmax()]
    assert cluster[1:cluster[0] + 1].tolist() == gen.CLUSTER[:k_slots - 1].tolist()
    if method == "max":
        assert (w_am == -1).any() and (w_am[4] == gen.CLUSTER[1]).sum() == c   # the tie: the lower slot
        assert not (w_am[4] == gen.CLUSTER[3]).any()
    else:
        assert not w_am.any()


@pytest.mark.gpu
def test_hip_roiaware_max_ignores_nan_and_minus_inf():
    import torch
    from pdanet_amd import roiaware_pool3d_utils as au
    feat = _KA_FEAT.copy()
    feat[0] = [np.nan, -np.inf]
    feat[2] = [-3, -np.inf]
    feat[1] = [-0.0, 0.0]
    feat[5] = [0.0, -0.0]                                              # -0 > +0 and +0 > -0 are both false: the lower slot stays
    w_am, w_sl, w_pf = np.zeros((1, 2, 2, 1, 2), I32), np.zeros((1, 2, 2, 1, 3), I32), np.zeros((1, 2, 2, 1, 2), F32)
    ref.roiaware_pool3d_forward(_KA_BOX, _KA_PTS, feat, w_am, w_sl, w_pf, 0)
    assert w_am[0, 0, 1, 0].tolist() == [2, -1] and w_am[0, 1, 1, 0].tolist() == [1, 1]
    am, sl, pf = (torch.zeros(a.shape, dtype=torch.int32 if a.dtype == I32 else torch.float32, device="cuda") for a in (w_am, w_sl, w_pf))
    au.roiaware_pool3d_cuda.forward(_t(_KA_BOX), _t(_KA_PTS), _t(feat), am, sl, pf, 0)
    assert np.array_equal(am.cpu().numpy(), w_am) and np.array_equal(sl.cpu().numpy(), w_sl)
    assert np.array_equal(_bits(pf.cpu().numpy()), _bits(w_pf))


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("k_slots", K_SLOTS)
@pytest.mark.parametrize("out_size", OUT_SIZES, ids=str)
@pytest.mark.parametrize("c", [3, 70])
@pytest.mark.parametrize("kind", ["exact", "generic"])
def test_hip_roiaware_backward(kind, c, out_size, k_slots, method):
    """max: grad_out holds small integers, every float32 sum is exact whatever its order: array_equal.
    avg: per element against the float64 sum s of the terms t_i = grad_out / count.  The device forms fl(1 / count) (one
    rounding), the product with grad_out (one rounding) and adds n such terms in float32 in some order (n - 1 roundings):
    |got - s| <= (n + 2) * 2^-24 * sum|t_i| to first order.  Derived, not measured."""
    import torch
    from pdanet_amd import roiaware_pool3d_utils as au
    grid, m = _grid(out_size), METHODS.index(method)
    w_sl = _ref_collect(kind, grid, k_slots)
    rng = np.random.default_rng(3)
    if method == "max":
        w_am = _ref_aware(kind, c, grid, k_slots, 0)[0]
        g = rng.integers(-4, 5, (6,) + grid + (c,)).astype(F32)
    else:
        w_am = np.zeros((6,) + grid + (c,), I32)
        g = rng.normal(size=(6,) + grid + (c,)).astype(F32)
    s, mag, n = ref.roiaware_pool3d_backward_terms(w_sl, w_am, g, gen.P, m)
    grad_in = torch.zeros((gen.P, c), device="cuda")
    assert au.roiaware_pool3d_cuda.backward(_t(w_sl), _t(w_am), _t(g), grad_in, m) == 1
    got = grad_in.cpu().numpy().astype(F64)
    assert n.max() >= 2                                                # overlapping boxes: genuine collisions
    if method == "max":
        assert np.array_equal(got, s)
    else:
        bound = (n + 2) * U * mag
        err = np.abs(got - s)
        print("avg backward %s: max error %.3e, max error / bound %.3f, addends per element up to %d"
              % ((kind, c, out_size, k_slots), err.max(), (err / np.maximum(bound, 1e-300)).max(), n.max()))
        assert (err <= bound).all()


@pytest.mark.gpu
@pytest.mark.parametrize("width", [0.0, 1.0])
@pytest.mark.parametrize("n_sample", [16, 512])
@pytest.mark.parametrize("c", [5, 130])
@pytest.mark.parametrize("kind", ["exact", "generic"])
def test_hip_roipoint_forward(kind, c, n_sample, width):
    from pdanet_amd import roipoint_pool3d_utils as pu
    inp = _point_inputs(kind)
    feat = inp["feat%d" % c]
    boxes = inp["boxes"].copy()
    boxes[..., 3:6] += F32(width)                                      # enlarge_box3d: float32 additions
    w_rows, w_flag = np.zeros((2, 5, n_sample, 3 + c), F32), np.zeros((2, 5), I32)
    ref.roipoint_pool3d_forward(inp["xyz"], boxes, feat, w_rows, w_flag, _contract())
    rows, flag = pu.RoIPointPool3d(n_sample, width)(_t(inp["xyz"]), _t(feat), _t(inp["boxes"]))
    assert tuple(rows.shape) == (2, 5, n_sample, 3 + c) and tuple(flag.shape) == (2, 5)
    assert np.array_equal(flag.cpu().numpy(), w_flag)
    assert np.array_equal(_bits(rows.cpu().numpy()), _bits(w_rows))
    # cnt = 0, 0 < cnt < S, cnt == S and cnt > S are all there
    counts = (inp["counts_wide"] if width else inp["counts"]).reshape(-1)
    assert (counts == 0).any() and ((counts > 0) & (counts < n_sample)).any() and (counts == n_sample).any() and (counts > n_sample).any()
    assert w_flag.sum() == (counts == 0).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["exact", "generic"])
def test_hip_points_in_boxes_cpu(kind):
    import torch
    from pdanet_amd import roiaware_pool3d_utils as au
    inp = _aware_inputs(kind)
    pts = inp["pts"].copy()
    pts[:3] = inp["rois"][1, :3] + np.array([[inp["rois"][1, 3] / 2 + 5e-3, 0, 0], [0, 0, 0], [0, 0, inp["rois"][1, 5] / 2 + 5e-3]], F32)
    want = np.zeros((6, gen.P), I32)
    ref.points_in_boxes_cpu(inp["rois"], pts, want)
    got = au.points_in_boxes_cpu(pts, inp["rois"])                     # numpy in, numpy out
    assert isinstance(got, np.ndarray) and got.dtype == I32 and np.array_equal(got, want)
    if kind == "exact":                                                # heading 0: 5e-3 m outside the x face is inside by 1e-2
        assert want[1, :3].tolist() == [1, 1, 0]
        assert not ref.in_box(pts[:1], inp["rois"][1], ref.MARGIN_GPU, _contract())[0][0]
    got = au.points_in_boxes_cpu(_t(pts), _t(inp["rois"]))             # tensors: the result stays on the input's device
    assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    got = au.points_in_boxes_cpu(torch.from_numpy(pts), torch.from_numpy(inp["rois"]))
    assert not got.is_cuda and np.array_equal(got.numpy(), want)


@pytest.mark.gpu
def test_two_runs_give_the_same_bits():
    from pdanet_amd import roipoint_pool3d_utils as pu
    inp = _aware_inputs("generic")
    for grid in ((12, 12, 12), (40, 40, 8)):                           # counters in LDS, counters in place
        for m in (0, 1):
            a, b = _gpu_aware(inp, 70, grid, 4, m), _gpu_aware(inp, 70, grid, 4, m)
            assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    p = _point_inputs("generic")
    runs = [pu.RoIPointPool3d(512, 1.0)(_t(p["xyz"]), _t(p["feat130"]), _t(p["boxes"])) for _ in range(2)]
    assert all(np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy())) for x, y in zip(*runs))


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_autograd_equals_a_direct_backward(method):
    import torch
    from pdanet_amd import roiaware_pool3d_utils as au
    inp = _aware_inputs("generic")
    rois, pts = _t(inp["rois"]).requires_grad_(True), _t(inp["pts"]).requires_grad_(True)
    feat = _t(inp["feat3"]).requires_grad_(True)
    out = au.RoIAwarePool3d((3, 4, 5), 8)(rois, pts, feat, pool_method=method)
    g = np.random.default_rng(9).integers(-4, 5, tuple(out.shape)).astype(F32)      # integers: the order of the atomics is invisible
    g = g * (1.0 if method == "max" else 840.0)                        # avg: counts up to 7 divide 840
    out.backward(_t(g))
    assert rois.grad is None and pts.grad is None
    sl, am, m = out.grad_fn.roiaware_pool3d_for_backward[:3]
    direct = torch.zeros_like(feat)
    au.roiaware_pool3d_cuda.backward(sl, am, _t(g), direct, m)
    assert sl[..., 0].max().item() <= 7 and feat.grad.abs().sum().item() > 0
    if method == "max":
        assert torch.equal(feat.grad, direct)
    else:                                                              # 840 / count is an integer only up to the rounding of 1 / count
        s, mag, n = ref.roiaware_pool3d_backward_terms(sl.cpu().numpy(), am.cpu().numpy(), g, gen.P, 1)
        for got in (feat.grad, direct):
            assert (np.abs(got.cpu().numpy().astype(F64) - s) <= (n + 2) * U * mag).all()


@pytest.mark.gpu
def test_roipoint_backward_is_not_implemented():
    from pdanet_amd import roipoint_pool3d_utils as pu
    inp = _point_inputs("exact")
    feat = _t(inp["feat5"]).requires_grad_(True)
    rows, _ = pu.RoIPointPool3d(16, 1.0)(_t(inp["xyz"]), feat, _t(inp["boxes"]))
    with pytest.raises(NotImplementedError):
        rows.sum().backward()


# ---------------------------------------------------------------- the reference's own Python composition -----------
@pytest.mark.gpu
def test_golden_reference_composition():
    """tests/golden/roi_pool.npz: the reference's RoIAwarePool3d (forward and backward, max and avg), RoIPointPool3d and
    points_in_boxes_cpu run on the CPU over the restatement (tests/golden/make_roi_pool_golden.py); inputs on the 1/8 lattice
    with heading 0, so either contraction mode gives the same bits."""
    from pdanet_amd import roiaware_pool3d_utils as au, roipoint_pool3d_utils as pu
    z = _golden()
    for tag in [str(t) for t in z["aware_cases"]]:
        ox, oy, oz, k, m = (int(v) for v in z[tag + "_args"])
        feat = _t(z["feat"]).requires_grad_(True)
        out = au.RoIAwarePool3d(ox if ox == oy == oz else (ox, oy, oz), k)(_t(z["rois"]), _t(z["pts"]), feat, pool_method=METHODS[m])
        sl, am = out.grad_fn.roiaware_pool3d_for_backward[:2]
        assert np.array_equal(sl.cpu().numpy(), z[tag + "_slots"]) and np.array_equal(am.cpu().numpy(), z[tag + "_argmax"])
        assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(z[tag + "_out"]))
        out.backward(_t(z[tag + "_grad_out"]))
        got = feat.grad.cpu().numpy()
        if m == 0:
            assert np.array_equal(got, z[tag + "_grad_in"])            # integer gradients: exact sums
        else:
            s, mag, n = ref.roiaware_pool3d_backward_terms(z[tag + "_slots"], z[tag + "_argmax"], z[tag + "_grad_out"], gen.P, 1)
            assert (np.abs(got.astype(F64) - s) <= (n + 2) * U * mag).all()
            # the file's own gradient is the same float64 sum rounded once
            assert (np.abs(z[tag + "_grad_in"].astype(F64) - s) <= U * np.abs(s)).all()
    for tag in [str(t) for t in z["point_cases"]]:
        s, w = int(z[tag + "_args"][0]), float(z[tag + "_args"][1])
        rows, flag = pu.RoIPointPool3d(s, w)(_t(z["xyz"]), _t(z["pfeat"]), _t(z["boxes"]))
        assert np.array_equal(flag.cpu().numpy(), z[tag + "_flag"]) and np.array_equal(_bits(rows.cpu().numpy()), _bits(z[tag + "_rows"]))
    assert np.array_equal(au.points_in_boxes_cpu(z["pts"], z["rois"]), z["mask"])


# ---------------------------------------------------------------- the uncontracted build ---------------------------
@pytest.mark.gpu
def test_exact_cases_with_the_uncontracted_build():
    """libpda_pointnet2_c0.so (PDA_LIB_PATH selects it at load time, as in tests/test_contract0.py) runs the exact cases of this
    file in a child process; the restatement follows the library's contraction mode."""
    lib = os.path.join(ROOT, "pdanet_amd", "libpda_pointnet2_c0.so")
    assert os.path.exists(lib), "build it: make -C pdanet_amd/csrc (or __graft_entry__.build())"
    env = dict(os.environ, PDA_LIB_PATH=lib, PDA_ROI_POOL_EXPECT_CONTRACT="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "(exact or golden or contract_mode) and not uncontracted"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    import re
    found = re.search(r"(\d+) passed", r.stdout)
    assert found and int(found.group(1)) >= 55, r.stdout[-500:]


@pytest.mark.gpu
def test_contract_mode_is_the_selected_one():
    assert _contract() == int(os.environ.get("PDA_ROI_POOL_EXPECT_CONTRACT", "1"))
