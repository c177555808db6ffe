"""PartA2FCHead and its input stage (pdanet_amd/parta2_head.py, csrc/parta2.hip pda_parta2_pool_*): the fused stage against the
composed path (PDA_PARTA2_POOL=composed: per-scene masks, two RoIAwarePool3d calls, nonzero, indexing) and against the
reference's own composition on the CPU (tests/golden/parta2.npz, make_parta2_golden.py).

Inputs (tests/golden/parta2_inputs.py): 2 scenes of 500 and 300 points with 16 channels, 3 RoIs a scene with an empty one and
a zero-padded row, pool sizes 4 and 12, MAX_POINTS_PER_VOXEL 8 with a 12-point cluster in one voxel, scores on both sides of
SEG_MASK_SCORE_THRESH 0.3.

Forward: coords, part rows and feature rows are BITWISE those of the composed path and of the fixture.  Gradients: the
composed order of work restated in float64 (roi_pool_restatement.py: the float32 kernels' decisions, the backward's terms
summed in float64) is the reference; the fused path may be off by FACTOR = 4 times the error of the composed float32 path on
the device, measured here as max |a - ref| / max |ref| (both add with float atomics).  The head end to end, on a tiny config
without dropout: everything the two paths compute from the same rows is bitwise equal (predictions, losses, the gradients of
the head's own parameters); the gradients that go back through the pooling differ by the order of their float atomics, at most
N = 4 terms an entry (one per sampled RoI of the scene), so by at most 2 (N - 1) 2^-24 of the sum of the terms' magnitudes,
itself at most N times the largest entry: 2 (N - 1) N 2^-24 = 1.4e-6 of it."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from pdanet_amd import _lib, build
from pdanet_amd.config import to_attr
from pdanet_amd.parta2_head import PartA2FCHead, parta2_pool, parta2_pool_composed
from pdanet_amd.roiaware_pool3d_utils import RoIAwarePool3d

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import parta2_inputs as inputs  # noqa: E402
import roi_pool_restatement as rpr  # noqa: E402

gpu = pytest.mark.gpu
FACTOR = 4.0
with open(os.path.join(HERE, "golden", "parta2_state_dict.json")) as _f:
    FIXTURE = json.load(_f)
ROI_CFG = FIXTURE['config']['MODEL']['ROI_HEAD']
GOLD = np.load(os.path.join(HERE, "golden", "parta2.npz"))
DATA = inputs.pool_inputs()
KEYS = ('rois', 'point_coords', 'point_features', 'point_part_offset', 'point_cls_scores')
F32, F64, I32 = np.float32, np.float64, np.int32


def tiny_cfg(pool_size=4, **over):
    cfg = json.loads(json.dumps(ROI_CFG))
    cfg.update(SEG_MASK_SCORE_THRESH=DATA['thresh'], SHARED_FC=[32], CLS_FC=[32], REG_FC=[32], DP_RATIO=0,
               ROI_AWARE_POOL={'POOL_SIZE': pool_size, 'NUM_FEATURES': 32, 'MAX_POINTS_PER_VOXEL': DATA['k_slots']})
    cfg['TARGET_CONFIG']['ROI_PER_IMAGE'] = 4
    cfg.update(over)
    return to_attr(cfg)


def rel(a, ref):
    a, ref = np.asarray(a, F64), np.asarray(ref, F64)
    assert a.shape == ref.shape
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_state_dict_is_the_references():
    head = PartA2FCHead(input_channels=16, model_cfg=to_attr(ROI_CFG), num_class=1)
    own = head.state_dict()
    assert [[k, list(v.shape)] for k, v in own.items()] == FIXTURE['PartA2FCHead']
    for name in ('conv_part', 'conv_rpn', 'shared_fc_layer', 'cls_layers', 'reg_layers', 'roiaware_pool3d_layer'):
        assert hasattr(head, name)
    assert isinstance(head.roiaware_pool3d_layer, RoIAwarePool3d) and head.roiaware_pool3d_layer.out_size == 12
    assert [c[0].indice_key for c in list(head.conv_part) + list(head.conv_rpn)] == list(PartA2FCHead.RCNN_KEYS)
    small = PartA2FCHead(input_channels=16, model_cfg=tiny_cfg(), num_class=1)
    small.load_state_dict({k: torch.zeros_like(v) for k, v in small.state_dict().items()}, strict=True)


def test_inputs_hold_every_case():
    for key in KEYS:
        assert GOLD['pool_' + key].tobytes() == DATA[key].tobytes()
    coords, scores = DATA['point_coords'], DATA['point_cls_scores']
    assert [int((coords[:, 0] == s).sum()) for s in (0, 1)] == [500, 300] and (np.diff(coords[:, 0]) >= 0).all()
    assert (scores < DATA['thresh']).sum() > 100 and (scores >= DATA['thresh']).sum() > 100 and not DATA['rois'][1, 2].any()
    c12 = GOLD['pool12_coords']
    per_roi = np.bincount(c12[:, 0], minlength=6)
    assert per_roi[2] == 0 and per_roi[5] == 0 and (per_roi[[0, 1, 3, 4]] > 0).all()             # the empty RoI and the zero row
    assert (np.diff(((c12[:, 0].astype(np.int64) * 12 + c12[:, 1]) * 12 + c12[:, 2]) * 12 + c12[:, 3]) > 0).all()   # nonzero()'s order


def test_refusals():
    with pytest.raises(NotImplementedError, match="submanifold"):
        PartA2FCHead(input_channels=16, model_cfg=tiny_cfg(), num_class=1).post_act_block(4, 16, 3, 'k', conv_type='inverseconv')
    z = torch.zeros
    args = (z(2, 3, 7), z(10, 4), z(10, 16), z(10, 3), z(10), 0.3)
    with pytest.raises(NotImplementedError, match="POOL_SIZE"):
        parta2_pool(*args, 17, 8)
    with pytest.raises(ValueError):
        parta2_pool(z(2, 3, 6), *args[1:], 4, 8)
    with pytest.raises(ValueError):
        parta2_pool(args[0], z(10, 3), *args[2:], 4, 8)
    with pytest.raises(ValueError):
        parta2_pool(*args[:3], z(9, 3), *args[4:], 4, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        parta2_pool(*args, 4, 8)
    head = PartA2FCHead(input_channels=16, model_cfg=tiny_cfg(), num_class=1)
    batch = dict(zip(KEYS, args[:5]))
    os.environ['PDA_PARTA2_POOL'] = 'neither'
    try:
        with pytest.raises(ValueError, match="PDA_PARTA2_POOL"):
            head.roiaware_pool(batch)
    finally:
        del os.environ['PDA_PARTA2_POOL']


def test_entry_points_validate_before_any_launch(lib):
    i64, f = ctypes.c_int64, ctypes.c_float
    err = lib.pda_last_error
    buf = ctypes.addressof((ctypes.c_double * 8)())
    assert lib.pda_parta2_pool_workspace_bytes(i64(6), 4) >= 6 * 64 * 16 and lib.pda_parta2_pool_workspace_bytes(i64(6), 17) == -1
    assert lib.pda_parta2_pool_workspace_bytes(i64(1 << 20), 16) == -1 and "pda_parta2_pool_workspace_bytes" in _lib.SIZE_QUERIES
    assert lib.pda_parta2_pool_segments(None, i64(-1), 2, None, None, None) == 1 and b"bad size" in err()
    assert lib.pda_parta2_pool_segments(None, i64(5), 2, None, None, None) == 1 and b"null" in err()
    assert lib.pda_parta2_pool_collect(None, None, None, None, 2, 3, i64(5), 17, 8, None) == 1 and b"bad size" in err()
    assert lib.pda_parta2_pool_collect(None, None, None, None, 2, 3, i64(5), 4, 0, None) == 1 and b"bad size" in err()
    assert lib.pda_parta2_pool_collect(None, None, None, None, 2, 3, i64(5), 4, 8, None) == 1 and b"null" in err()
    assert lib.pda_parta2_pool_collect(None, None, None, None, 0, 3, i64(5), 4, 8, None) == 0                 # no RoIs
    assert lib.pda_parta2_pool_sparsify(None, None, 3, 0, None, f(0.3), None, None, None, None, None, i64(6), i64(5), 0, 8, None) == 1 \
        and b"bad size" in err()
    assert lib.pda_parta2_pool_sparsify(None, None, 2, 0, None, f(0.3), None, None, None, None, None, i64(6), i64(5), 4, 8, None) == 1 \
        and b"stride" in err()
    assert lib.pda_parta2_pool_sparsify(None, None, 3, 0, None, f(0.3), None, None, None, None, None, i64(6), i64(5), 4, 8, None) == 1 \
        and b"null" in err()
    assert lib.pda_parta2_pool_sparsify(None, None, 3, 0, None, f(0.3), buf + 8, buf, None, None, None, i64(6), i64(5), 4, 8, None) == 1 \
        and b"aligned" in err()
    assert lib.pda_parta2_pool_features(None, None, None, None, None, None, i64(6), i64(5), 0, 4, 8, None) == 1 and b"channels" in err()
    assert lib.pda_parta2_pool_features(None, None, None, None, None, None, i64(6), i64(5), 16, 4, 8, None) == 1 and b"null" in err()
    assert lib.pda_parta2_pool_features(None, None, None, None, None, None, i64(0), i64(5), 16, 4, 8, None) == 0
    assert lib.pda_parta2_pool_bwd(None, None, None, None, f(0.3), None, None, None, None, i64(-1), i64(5), 16, 8, None) == 1 \
        and b"bad size" in err()
    assert lib.pda_parta2_pool_bwd(None, None, None, None, f(0.3), buf, None, None, None, i64(3), i64(5), 16, 8, None) == 1 \
        and b"null" in err()
    assert lib.pda_parta2_pool_bwd(None, None, None, None, f(0.3), None, None, None, None, i64(0), i64(5), 16, 8, None) == 0


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def device_inputs(grad=False):
    t = {k: dev(DATA[k]) for k in KEYS}
    if grad:
        t['point_features'].requires_grad_(True)
        t['point_part_offset'].requires_grad_(True)
    return t


def run_path(path, pool_size, grad=False, weights=None):
    t = device_inputs(grad)
    args = [t[k] for k in KEYS] + [DATA['thresh']]
    if path == 'fused':
        coords, part, feat = parta2_pool(*args, pool_size, DATA['k_slots'], check=True)
    else:
        coords, part, feat = parta2_pool_composed(RoIAwarePool3d(pool_size, DATA['k_slots']), *args)
    grads = None
    if grad:
        ((part * dev(weights[0])).sum() + (feat * dev(weights[1])).sum()).backward()
        grads = [t['point_part_offset'].grad.cpu().numpy(), t['point_features'].grad.cpu().numpy()]
    torch.cuda.synchronize()
    return coords.cpu().numpy(), part.detach().cpu().numpy(), feat.detach().cpu().numpy(), grads


@gpu
@pytest.mark.parametrize("pool_size", [4, 12])
def test_gpu_forward_is_bitwise_the_composed_path_and_the_fixture(pool_size):
    fused, composed = run_path('fused', pool_size), run_path('composed', pool_size)
    want = [GOLD['pool%d_%s' % (pool_size, k)] for k in ('coords', 'part', 'rpn')]
    assert fused[0].dtype == I32 and fused[0].shape == (len(want[0]), 4)                           # n_live = nonzero()'s count
    for name, a, b, w in zip(('coords', 'part rows', 'feature rows'), fused, composed, want):
        assert a.shape == b.shape == w.shape, name
        assert a.tobytes() == b.tobytes(), name
        assert a.tobytes() == w.tobytes(), name
    again = run_path('fused', pool_size)                                                           # two runs: the same bits
    assert all(a.tobytes() == b.tobytes() for a, b in zip(fused[:3], again[:3]))


def restated_gradients(pool_size, coords, weights):
    """The composed order of work with the float32 restatement of the kernels (per scene: the avg pool's slots, the max pool's
    argmax), the backward's terms added in float64: d/d point_part_offset and d/d point_features of
    sum(part rows * weights[0]) + sum(feature rows * weights[1])."""
    o, k, thresh = pool_size, DATA['k_slots'], F32(DATA['thresh'])
    pc, feats, scores = DATA['point_coords'], DATA['point_features'], DATA['point_cls_scores']
    part = np.concatenate([DATA['point_part_offset'], scores[:, None]], 1).astype(F32)
    part[scores < thresh, 0:3] = 0
    g_off, g_feat = np.zeros((len(pc), 3), F64), np.zeros(feats.shape, F64)
    n_roi = DATA['rois'].shape[1]
    for s in range(DATA['rois'].shape[0]):
        rows = np.nonzero(pc[:, 0] == s)[0]
        rois, xyz = np.ascontiguousarray(DATA['rois'][s, :, :7]), np.ascontiguousarray(pc[rows, 1:4])
        live = (coords[:, 0] >= s * n_roi) & (coords[:, 0] < (s + 1) * n_roi)
        at = (coords[live, 0] - s * n_roi, coords[live, 1], coords[live, 2], coords[live, 3])
        for method, f, w, width in ((1, part[rows], weights[0], 4), (0, feats[rows], weights[1], feats.shape[1])):
            pooled, argmax = np.zeros((n_roi, o, o, o, width), F32), np.zeros((n_roi, o, o, o, width), I32)
            slots = np.zeros((n_roi, o, o, o, k), I32)
            rpr.roiaware_pool3d_forward(rois, xyz, np.ascontiguousarray(f), argmax, slots, pooled, method)
            grad_out = np.zeros(pooled.shape, F64)
            grad_out[at] = w[live]
            terms, _, _ = rpr.roiaware_pool3d_backward_terms(slots, argmax, grad_out, len(rows), method)
            if method == 1:
                terms[scores[rows] < thresh] = 0
                g_off[rows] = terms[:, :3]
            else:
                g_feat[rows] = terms
    return [g_off, g_feat]


@gpu
@pytest.mark.parametrize("pool_size", [4, 12])
def test_gpu_gradients(pool_size):
    n = len(GOLD['pool%d_coords' % pool_size])
    rng = np.random.default_rng(40 + pool_size)
    weights = [rng.standard_normal((n, 4)).astype(F32), rng.standard_normal((n, inputs.POOL_CHANNELS)).astype(F32)]
    coords, _, _, fused = run_path('fused', pool_size, True, weights)
    _, _, _, composed = run_path('composed', pool_size, True, weights)
    ref = restated_gradients(pool_size, coords, weights)
    for what, a, c, r in zip(("point_part_offset", "point_features"), fused, composed, ref):
        assert np.abs(r).max() > 0
        e_fused, e_composed = rel(a, r), rel(c, r)
        print("pool", pool_size, "gradient of", what, "fused err", e_fused, "composed float32 device err", e_composed)
        assert e_fused <= FACTOR * e_composed, what
    masked = DATA['point_cls_scores'] < DATA['thresh']
    assert not fused[0][masked].any() and fused[0][~masked].any()                                  # the mask reaches the gradient


def head_batch(training, rois=None):
    t = device_inputs(training)
    rois = DATA['rois'] if rois is None else rois
    batch = {'batch_size': 2, 'rois': dev(rois), 'roi_scores': torch.zeros(2, 3, device='cuda'),
             'roi_labels': torch.ones(2, 3, dtype=torch.long, device='cuda'), 'has_class_labels': False, 'roi_target_seed': 5}
    batch.update({k: t[k] for k in KEYS[1:]})
    if training:
        gt = np.zeros((2, 2, 8), F32)
        gt[:, :, :7] = DATA['rois'][:, :2]
        gt[:, :, 3:6] *= 1.05
        gt[:, :, 7] = 1
        batch['gt_boxes'] = dev(gt)
    return batch, t


def run_head(path, model, training, rois=None):
    os.environ['PDA_PARTA2_POOL'] = path
    try:
        head = PartA2FCHead(input_channels=inputs.POOL_CHANNELS, model_cfg=tiny_cfg(), num_class=1).cuda()
        head.load_state_dict(model)
        head.train(training)
        batch, t = head_batch(training, rois)
        if not training:
            with torch.no_grad():
                out = head(batch)
            return out['batch_cls_preds'], out['batch_box_preds']
        head(batch)
        ret = head.forward_ret_dict
        loss, tb = head.get_loss()
        loss.backward()
        torch.cuda.synchronize()
        return ret, loss.detach(), tb, {k: p.grad for k, p in head.named_parameters()}, [t['point_part_offset'].grad, t['point_features'].grad]
    finally:
        del os.environ['PDA_PARTA2_POOL']


@pytest.fixture
def deterministic_dense_kernels():
    """The head's Conv1d stacks run through MIOpen, whose default kernels add with float atomics: two runs of ONE path on one
    input differ in the last bits from shared_fc_layer on (measured on MI355X: everything up to dense() is the same bits, the
    class scores move by 1e-8).  Bit-equality between the paths asks for its deterministic kernels, as in
    tests/test_sparse_padded.py."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


def head_weights():
    torch.manual_seed(3)
    return PartA2FCHead(input_channels=inputs.POOL_CHANNELS, model_cfg=tiny_cfg(), num_class=1).state_dict()


@gpu
def test_gpu_head_eval_is_bitwise_equal_between_the_paths(deterministic_dense_kernels):
    model = head_weights()
    fused, composed = run_head('fused', model, False), run_head('composed', model, False)
    assert fused[0].shape == (2, 3, 1) and fused[1].shape == (2, 3, 7)
    assert torch.equal(fused[0], composed[0]) and torch.equal(fused[1], composed[1]) and torch.isfinite(fused[1]).all()


@gpu
def test_gpu_head_train_agrees_between_the_paths(deterministic_dense_kernels):
    model = head_weights()
    f_ret, f_loss, f_tb, f_par, f_in = run_head('fused', model, True)
    c_ret, c_loss, c_tb, c_par, c_in = run_head('composed', model, True)
    assert set(f_tb) == {'rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner', 'rcnn_loss'}
    assert torch.equal(f_ret['rois'], c_ret['rois']) and (f_ret['rcnn_cls_labels'] >= 0).any()      # the same sampled targets
    # the same rows in, the same code after them: bitwise equal
    assert torch.equal(f_ret['rcnn_cls'], c_ret['rcnn_cls']) and torch.equal(f_ret['rcnn_reg'], c_ret['rcnn_reg'])
    assert torch.equal(f_loss, c_loss) and torch.isfinite(f_loss)
    assert set(f_par) == set(c_par) and all(g is not None and torch.equal(g, c_par[k]) for k, g in f_par.items())
    # back through the pooling: the order of at most N = 4 float atomics an entry (ROI_PER_IMAGE)
    for what, a, c in zip(("point_part_offset", "point_features"), f_in, c_in):
        err = rel(a.cpu().numpy(), c.cpu().numpy())
        print("head train gradient of", what, "fused against composed", err)
        assert c.abs().max() > 0 and err <= 2 * (4 - 1) * 4 * 2.0 ** -24


@gpu
def test_gpu_all_rois_empty_takes_the_fake_sparse_idx_branch():
    far = DATA['rois'].copy()
    far[:, :, 0] += 500.0                                                    # nothing inside any RoI
    model = head_weights()
    for path in ('fused', 'composed'):
        ret, loss, tb, par, _ = run_head(path, model, True, far)
        assert torch.isfinite(ret['rcnn_cls']).all() and torch.isfinite(ret['rcnn_reg']).all() and torch.isfinite(loss)
        assert (ret['rcnn_cls_labels'] == -1).all() and (ret['reg_valid_mask'] == -1).all()
        cls, box = run_head(path, model, False, far)
        assert torch.isfinite(cls).all() and torch.isfinite(box).all()
    # fewer than 3 live voxels, one of them voxel (0, 0, 0) of a RoI: its rows stand in, zeros elsewhere
    coords = torch.tensor([[1, 0, 0, 0], [2, 1, 0, 3]], dtype=torch.int32, device='cuda')
    part, feat = torch.ones(2, 4, device='cuda'), torch.full((2, 16), 2.0, device='cuda')
    fc, fp, ff = PartA2FCHead.fake_sparse_idx(coords, part, feat, 4)
    assert fc.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0], [3, 0, 0, 0]]
    assert fp.sum(1).tolist() == [0, 4, 0, 0] and ff.sum(1).tolist() == [0, 32, 0, 0]


@gpu
def test_gpu_check_finds_rows_that_are_not_scene_major():
    t = device_inputs()
    swapped = t['point_coords'].clone()
    swapped[[0, 799]] = swapped[[799, 0]]
    args = [t[k] for k in KEYS[2:]] + [DATA['thresh'], 4, DATA['k_slots']]
    with pytest.raises(ValueError, match="scene-major"):
        parta2_pool(t['rois'], swapped, *args, check=True)
    coords, _, _ = parta2_pool(t['rois'], swapped, *args)                    # unchecked: wrong rows, but rows of the point set
    assert coords.shape[1] == 4
    # no points, and no RoIs: nothing is live
    none = parta2_pool(t['rois'], swapped[:0], t['point_features'][:0], t['point_part_offset'][:0], t['point_cls_scores'][:0],
                       DATA['thresh'], 4, DATA['k_slots'])
    assert [tuple(x.shape) for x in none] == [(0, 4), (0, 4), (0, 16)]
    none = parta2_pool(t['rois'][:, :0], *[t[k] for k in KEYS[1:]], DATA['thresh'], 4, DATA['k_slots'])
    assert [tuple(x.shape) for x in none] == [(0, 4), (0, 4), (0, 16)]
