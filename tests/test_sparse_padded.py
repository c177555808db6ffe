"""The padded, read-free form of the sparse convolutions (pdanet_amd/spconv_utils.py, csrc/bn_relu.hip
pda_bn_relu_*_counted, csrc/sparse_conv_index.hip pda_spconv_index_*_counted, voxel_utils.collate_voxels_padded).

CPU part: the new entries are exported and bound, their argument validation, the Python refusals, the state-dict keys.
GPU part: the counted index stage integer-exact against the compact build; the counted BatchNorm against
torch.nn.functional.batch_norm in float64 on the live rows; convolution layers padded against compact, bit for bit on small
integers; the two backbones against the dense float64 restatement (tests/golden/sparse_conv_restatement.py); SECONDNet's
training iteration without a host read and replayed from one graph; the padded collate against collate_voxels.

Tolerances.  BatchNorm and the backbones: the float32 CPU computation of the same thing is run next to the float64
reference, its error max |a - ref| / max |ref| is measured here, and the device may be off by 4 times that (the rule of
tests/test_second_net.py); both figures are printed, BASELINE.md section 4 records them.  A BatchNorm over one live row has
no torch reference (torch raises): there the result is known in closed form (y = beta, running_mean moves towards the row,
the variance is 0) and a float32 result may differ from it by one rounding, 2^-23 relative.  Everything else is exact."""
import copy
import ctypes
import gc
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pdanet_amd import _lib, build, spconv_utils as sp
from pdanet_amd.config import to_attr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import sparse_conv_restatement as rs  # noqa: E402

gpu = pytest.mark.gpu
NEW_ENTRIES = ["pda_bn_relu_fwd_counted", "pda_bn_relu_bwd_counted", "pda_spconv_index_subm_counted",
               "pda_spconv_index_strided_counted"]
GRID, BATCH, LIVE = (9, 16, 16), 2, 300
CAPS = (300, 320, 512)          # a full tensor, a partial last 64-row tile, many dead tiles
# name -> (kernel, stride, padding, subm)
GEOMS = {'subm3': (3, 1, 1, True), 's2p1': (3, 2, 1, False), 'k311': ((3, 1, 1), (2, 1, 1), 0, False)}
FACTOR = 4.0


def sites():
    """LIVE rows (b, z, y, x) at distinct random cells of the two scenes, shuffled."""
    D, H, W = GRID
    rng = np.random.default_rng(21)
    cells = rng.choice(BATCH * D * H * W, LIVE, replace=False)
    return np.stack([cells // (D * H * W), (cells // (H * W)) % D, (cells // W) % H, cells % W], axis=1).astype(np.int32)


SITES = sites()


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_new_entries_are_exported_and_bound(lib):
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert (sp.FLAG_DUPLICATE, sp.FLAG_OUTSIDE, sp.FLAG_OVERFLOW, sp.FLAG_FEW_ROWS) == (1, 2, 4, 8)


def test_argument_validation_without_gpu(lib):
    i64, f = ctypes.c_int64, ctypes.c_float
    words = (ctypes.c_int32 * 64)()
    buf = ctypes.addressof(words)          # 16-byte alignment is not promised: the size checks come first
    err = lib.pda_last_error
    fwd, bwd = lib.pda_bn_relu_fwd_counted, lib.pda_bn_relu_bwd_counted
    # null pointers
    assert fwd(None, None, None, None, None, None, None, None, i64(8), 16, f(1e-3), f(0.01), None, None, 1, 1, None) == 1 and b"null" in err()
    assert bwd(None, None, None, None, None, None, None, None, None, i64(8), 16, None, 1, 1, None) == 1 and b"null" in err()
    assert lib.pda_spconv_index_subm_counted(None, i64(4), None, 1, 5, 12, 10, 3, 3, 3, None, None, None, None) == 1 and b"null" in err()
    assert lib.pda_spconv_index_strided_counted(None, i64(4), None, 1, 5, 12, 10, 3, 3, 3, 2, 2, 2, 1, 1, 1, i64(8), None, None, None,
                                                None, None, None, None) == 1 and b"null" in err()
    # c out of range
    for c in (0, 2, 24, 2048):
        assert fwd(buf, buf, buf, buf, buf, buf, buf, buf, i64(8), c, f(1e-3), f(0.01), buf, buf, 1, 1, None) == 1 and b"C = " in err()
        assert bwd(buf, buf, buf, buf, buf, buf, buf, buf, buf, i64(8), c, buf, 1, 1, None) == 1 and b"C = " in err()
    # rows < 0, cap < 0
    assert fwd(buf, buf, buf, buf, buf, buf, buf, buf, i64(-1), 16, f(1e-3), f(0.01), buf, buf, 1, 1, None) == 1 and b"rows" in err()
    assert bwd(buf, buf, buf, buf, buf, buf, buf, buf, buf, i64(-1), 16, buf, 1, 1, None) == 1 and b"rows" in err()
    assert lib.pda_spconv_index_subm_counted(buf, i64(-1), buf, 1, 5, 12, 10, 3, 3, 3, buf, buf, buf, None) == 1 and b"bad size" in err()
    assert lib.pda_spconv_index_strided_counted(buf, i64(-1), buf, 1, 5, 12, 10, 3, 3, 3, 2, 2, 2, 1, 1, 1, i64(8), buf, buf, buf, buf,
                                                buf, buf, None) == 1 and b"bad size" in err()
    assert lib.pda_spconv_index_strided_counted(buf, i64(4), buf, 1, 5, 12, 10, 3, 3, 3, 2, 2, 2, 1, 1, 1, i64(-1), buf, buf, buf, buf,
                                                buf, buf, None) == 1 and b"cap" in err()
    # eval mode needs the running statistics; an empty capacity is PDA_OK and touches nothing
    assert fwd(buf, buf, buf, None, None, buf, buf, buf, i64(8), 16, f(1e-3), f(0.01), buf, buf, 1, 0, None) == 1 and b"running" in err()
    assert lib.pda_spconv_index_subm_counted(None, i64(0), None, 1, 5, 12, 10, 3, 3, 3, None, None, None, None) == 0
    assert lib.pda_spconv_index_strided_counted(None, i64(0), None, 1, 5, 12, 10, 3, 3, 3, 2, 2, 2, 1, 1, 1, i64(0), None, None, None,
                                                None, None, None, None) == 0


def test_python_refuses_cpu_tensors_and_bad_counts():
    from pdanet_amd.voxel_utils import collate_voxels_padded
    with pytest.raises(RuntimeError, match="no CPU path"):
        collate_voxels_padded(torch.zeros(2, 8, 5, 4), torch.zeros(2, 8, 3, dtype=torch.int32), torch.zeros(2, 8, dtype=torch.int32),
                              torch.zeros(2, dtype=torch.int32))
    one = torch.zeros(1, dtype=torch.int32)
    x = sp.SparseConvTensor(torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32), GRID, 1, num_active=one)
    assert x.status is not None and x.status.dtype == torch.int32 and x.replace_feature(x.features).num_active is one
    with pytest.raises(RuntimeError, match="no CPU path"):
        sp.SubMConv3d(4, 16, 3, indice_key='a')(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sp.build_strided_rulebook(x.indices, GRID, 1, 3, 2, 1, count=one, status=one)
    for bad in (torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(1), 3):
        with pytest.raises(ValueError, match="num_active"):
            sp.SparseConvTensor(torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32), GRID, 1, num_active=bad)
    with pytest.raises(ValueError, match="status"):
        sp.SparseConvTensor(torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32), GRID, 1, num_active=one,
                            status=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="status"):
        sp.SparseConvTensor(torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32), GRID, 1, status=one)


def test_two_stage_detectors_refuse_a_padded_batch():
    from pdanet_amd.pv_rcnn import PVRCNN
    from pdanet_amd.second_net_iou import SECONDNetIoU
    from pdanet_amd.voxel_rcnn import VoxelRCNN
    for cls, fixture in ((SECONDNetIoU, "second_iou_state_dict.json"), (VoxelRCNN, "voxel_rcnn_state_dict.json"),
                         (PVRCNN, "pv_rcnn_state_dict.json")):
        with open(os.path.join(HERE, "golden", fixture)) as f:
            cfg = json.load(f)['config']
        model = cls(to_attr(cfg['MODEL']), 3, cfg['dataset'])
        with pytest.raises(NotImplementedError, match="voxel_num_active"):
            model({'voxel_num_active': torch.zeros(1, dtype=torch.int32), 'batch_size': 2})


def test_state_dict_keys_do_not_move():
    from pdanet_amd.second_net import SECONDNet
    from pdanet_amd.spconv_backbone import VoxelBackBone8x, VoxelResBackBone8x
    with open(os.path.join(HERE, "golden", "second_state_dict.json")) as f:
        ref = json.load(f)
    cfg = ref['config']
    for name, cls in (('VoxelBackBone8x', VoxelBackBone8x), ('VoxelResBackBone8x', VoxelResBackBone8x)):
        m = cls(to_attr(dict(cfg['MODEL']['BACKBONE_3D'], PADDED_CAPS={'spconv2': 64})), 4, cfg['grid_size'])
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == ref[name]
    m = SECONDNet(to_attr(cfg['MODEL']), 3, cfg['dataset'])
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == ref['SECONDNet']


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def word(v=0):
    return torch.tensor([v], dtype=torch.int32).cuda()


def padded_indices(live_rows, cap, dead=None):
    """(cap, 4) int32 on the device: the live rows, then `dead` (default -1) repeated."""
    idx = np.full((cap, 4), -1, np.int32)
    idx[:len(live_rows)] = live_rows
    if dead is not None:
        idx[len(live_rows):] = dead
    return dev(idx)


def compact_book(rows, name, **kw):
    k, s, p, subm = GEOMS[name]
    ind = dev(np.asarray(rows, np.int32))
    if subm:
        return sp.build_subm_rulebook(ind, GRID, BATCH, k)
    return sp.build_strided_rulebook(ind, GRID, BATCH, k, s, p, **kw)


def padded_book(ind, count, status, name, **kw):
    k, s, p, subm = GEOMS[name]
    if subm:
        return sp.build_subm_rulebook(ind, GRID, BATCH, k, count=count, status=status)
    return sp.build_strided_rulebook(ind, GRID, BATCH, k, s, p, count=count, status=status, **kw)


@gpu
@pytest.mark.parametrize("name", list(GEOMS))
def test_gpu_index_equals_the_compact_build(name):
    subm = GEOMS[name][3]
    ref = compact_book(SITES, name)
    for cap in CAPS:
        status = word()
        book = padded_book(padded_indices(SITES, cap), word(LIVE), status, name)
        assert book.n_in == cap and int(status) == 0
        if subm:
            assert torch.equal(book.nbr_out[:LIVE], ref.nbr_out) and (book.nbr_out[LIVE:] == -1).all()
            continue
        n = ref.n_out
        assert book.count_out.tolist() == [n] and book.n_out >= n and book.out_shape == ref.out_shape
        assert torch.equal(book.out_indices[:n], ref.out_indices) and (book.out_indices[n:] == -1).all()
        assert torch.equal(book.nbr_out[:n], ref.nbr_out) and (book.nbr_out[n:] == -1).all()
        assert torch.equal(book.nbr_in[:LIVE], ref.nbr_in) and (book.nbr_in[LIVE:] == -1).all()
        again = padded_book(padded_indices(SITES, cap), word(LIVE), status, name)          # two runs give the same bits
        assert all(torch.equal(getattr(again, a), getattr(book, a)) for a in ('out_indices', 'nbr_out', 'nbr_in', 'count_out'))


@gpu
def test_gpu_index_overflow_keeps_the_smallest_keys():
    ref = compact_book(SITES, 's2p1')
    cap = ref.n_out - 7
    status = word()
    book = padded_book(padded_indices(SITES, 320), word(LIVE), status, 's2p1', cap=cap)
    assert int(status) == sp.FLAG_OVERFLOW and book.count_out.tolist() == [cap] and book.n_out == cap
    assert torch.equal(book.out_indices, ref.out_indices[:cap]) and torch.equal(book.nbr_out, ref.nbr_out[:cap])
    kept = torch.where(ref.nbr_in < cap, ref.nbr_in, torch.full_like(ref.nbr_in, -1))          # taps into dropped rows are gone
    assert torch.equal(book.nbr_in[:LIVE], kept) and (book.nbr_in[LIVE:] == -1).all()


@gpu
def test_gpu_index_flags_come_from_live_rows_only():
    D, H, W = GRID
    for name in ('subm3', 's2p1'):
        ref = compact_book(SITES, name)
        status = word()
        book = padded_book(padded_indices(SITES, 320, dead=SITES[5]), word(0), status, name)          # no live row at all
        assert int(status) == 0 and (book.nbr_out == -1).all()
        if name == 's2p1':
            assert book.count_out.tolist() == [0] and (book.out_indices == -1).all() and (book.nbr_in == -1).all()
        for bad, flag in ((SITES[17], sp.FLAG_DUPLICATE), ([0, D, 0, 0], sp.FLAG_OUTSIDE), ([BATCH, 0, 0, 0], sp.FLAG_OUTSIDE),
                          ([0, 0, -1, 0], sp.FLAG_OUTSIDE)):
            live = np.concatenate([SITES, np.asarray([bad], np.int32)])
            status = word()
            padded_book(padded_indices(live, 320), word(LIVE + 1), status, name)          # among the live rows: flagged
            assert int(status) == flag, (name, bad)
            status = word()
            book = padded_book(padded_indices(live, 320, dead=bad), word(LIVE), status, name)          # among the dead rows: not
            assert int(status) == 0, (name, bad)
            assert torch.equal(book.nbr_out[:ref.n_out], ref.nbr_out)
        status = word(sp.FLAG_FEW_ROWS)                                    # the word is ORed into, never cleared
        padded_book(padded_indices(np.concatenate([SITES, SITES[:1]]), 320), word(LIVE + 1), status, name)
        assert int(status) == sp.FLAG_FEW_ROWS | sp.FLAG_DUPLICATE


# ---- counted BatchNorm ---------------------------------------------------------------------------------------------------------
BN_SIZES = [(0, 64), (1, 64), (2, 64), (255, 256), (257, 1024), (1024, 1024)]
EPS, MOMENTUM = 1e-3, 0.01


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape
    return float(np.abs(a - ref).max(initial=0) / max(np.abs(ref).max(initial=0), 1e-300))


def bn_inputs(c, live, cap, seed):
    rng = np.random.default_rng(seed)
    d = {'x': rng.standard_normal((cap, c)) * 2 + 0.5, 'go': rng.standard_normal((cap, c)), 'w': rng.random(c) + 0.5,
         'b': rng.standard_normal(c) * 0.3, 'rm': rng.standard_normal(c) * 0.1, 'rv': rng.random(c) + 0.5}
    return {k: v.astype(np.float32) for k, v in d.items()}


def bn_torch(d, live, relu, training, dtype):
    """F.batch_norm (+ ReLU) on the live rows on the CPU: y, grad_x, grad_w, grad_b, running_mean, running_var."""
    t = lambda k: torch.tensor(d[k], dtype=dtype)
    x, w, b = t('x')[:live].requires_grad_(True), t('w').requires_grad_(True), t('b').requires_grad_(True)
    rm, rv = t('rm'), t('rv')
    y = F.batch_norm(x, rm, rv, w, b, training, MOMENTUM, EPS)
    y = torch.relu(y) if relu else y
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), t('go')[:live])
    return [v.detach().numpy() for v in (y, gx, gw, gb, rm, rv)]


def bn_one_row(d, relu):
    """Training mode over one row in closed form: mean = the row, variance 0 (biased and, by bn_finalize_fwd_kernel's rule, in
    the running update too); x_hat = 0, so y = beta, grad_x = 0, grad_gamma = 0 and grad_beta = the masked gradient."""
    f = lambda k: d[k].astype(np.float64)
    y = f('b')[None]
    dyh = f('go')[:1] * ((y > 0) if relu else 1.0)
    y = np.maximum(y, 0) if relu else y
    return [y, np.zeros_like(y), np.zeros_like(f('w')), dyh[0], (1 - MOMENTUM) * f('rm') + MOMENTUM * f('x')[0], (1 - MOMENTUM) * f('rv')]


def bn_device(d, live, cap, relu, training, dead_fill=None):
    c = d['x'].shape[1]
    bn = torch.nn.BatchNorm1d(c, eps=EPS, momentum=MOMENTUM).cuda().train(training)
    with torch.no_grad():
        bn.weight.copy_(dev(d['w'])), bn.bias.copy_(dev(d['b'])), bn.running_mean.copy_(dev(d['rm'])), bn.running_var.copy_(dev(d['rv']))
    x, go = d['x'].copy(), d['go'].copy()
    if dead_fill is not None:
        x[live:], go[live:] = dead_fill, dead_fill[::-1]
    x = dev(x).requires_grad_(True)
    status = word()
    y = sp.counted_batch_norm(bn, x, word(live), status, relu=relu)
    gx, gw, gb = torch.autograd.grad(y, (x, bn.weight, bn.bias), dev(go))
    out = [t.detach().cpu().numpy() for t in (y, gx, gw, gb, bn.running_mean, bn.running_var)]
    return out, int(status), int(bn.num_batches_tracked)


@gpu
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
@pytest.mark.parametrize("c", [16, 128])
def test_gpu_counted_batch_norm(c, relu, training):
    names = ("y", "grad_x", "grad_gamma", "grad_beta", "running_mean", "running_var")
    for live, cap in BN_SIZES:
        d = bn_inputs(c, live, cap, 1000 + c + live)
        got, status, tracked = bn_device(d, live, cap, relu, training)
        assert status == (sp.FLAG_FEW_ROWS if training and live < 2 else 0), (live, cap)
        assert tracked == (1 if training else 0)
        for a in got[:2]:
            assert a.shape == (cap, c) and not a[live:].any(), (live, cap)                  # dead rows: exact zeros
        live_got = [got[0][:live], got[1][:live]] + got[2:]
        if training and live == 0:
            assert not got[2].any() and not got[3].any()
            assert np.array_equal(got[4], d['rm']) and np.array_equal(got[5], d['rv'])      # the running statistics stay
        elif training and live == 1:
            for what, a, r in zip(names, live_got, bn_one_row(d, relu)):
                assert np.abs(a - r).max() <= 2.0 ** -23 * max(np.abs(r).max(), 1e-300), (what, live, cap)
        else:
            ref, f32 = bn_torch(d, live, relu, training, torch.float64), bn_torch(d, live, relu, training, torch.float32)
            for what, a, r, c32 in zip(names, live_got, ref, f32):
                if not training and what.startswith("running"):
                    assert np.array_equal(a, d['rm' if what == "running_mean" else 'rv'])
                    continue
                e_dev, e_f32 = rel(a, r), rel(c32, r)
                print("counted bn C=%d live=%d cap=%d relu=%d training=%d %s device err %.3g float32 CPU err %.3g"
                      % (c, live, cap, relu, training, what, e_dev, e_f32))
                assert e_dev <= FACTOR * e_f32, (what, live, cap, e_dev, e_f32)
        # the same bits from run to run, and whatever the dead rows of x and grad_y hold
        for fill in (None, np.array([np.nan, np.inf, -np.inf, 1e30] * (c // 4), np.float32)):
            again, status2, _ = bn_device(d, live, cap, relu, training, dead_fill=fill)
            assert status2 == status
            for what, a, b in zip(names, got, again):
                assert a.tobytes() == b.tobytes(), (what, live, cap, fill is not None)


# ---- convolution layers, padded against compact ---------------------------------------------------------------------------------
def small_ints(rng, shape):
    return rng.integers(-2, 3, shape).astype(np.float32)


@gpu
def test_gpu_conv_layers_padded_equal_compact_bits():
    rng = np.random.default_rng(77)
    cap = 512
    f = small_ints(rng, (LIVE, 16))
    w1, b1, w2 = small_ints(rng, (32, 3, 3, 3, 16)), small_ints(rng, (32,)), small_ints(rng, (32, 3, 3, 3, 32))
    conv1, conv2 = sp.SubMConv3d(16, 32, 3, indice_key='a').cuda(), sp.SparseConv3d(32, 32, 3, 2, 1, bias=False, indice_key='b').cuda()
    with torch.no_grad():
        conv1.weight.copy_(dev(w1)), conv1.bias.copy_(dev(b1)), conv2.weight.copy_(dev(w2))
    params = (conv1.weight, conv1.bias, conv2.weight)

    def run(x, go_of):
        y = conv2(conv1(x))
        go = go_of(y)
        return (y,) + torch.autograd.grad(y.features, (x.features,) + params, go)

    ft = dev(f).requires_grad_(True)
    y, *g_compact = run(sp.SparseConvTensor(ft, dev(SITES), GRID, BATCH), lambda y: dev(small_ints(np.random.default_rng(5), tuple(y.features.shape))))
    n_out = y.features.shape[0]
    go = small_ints(np.random.default_rng(5), (n_out, 32))

    fp = np.full((cap, 16), 3.0, np.float32)          # dead features: never read
    fp[:LIVE] = f
    fpt = dev(fp).requires_grad_(True)
    status = word()
    x = sp.SparseConvTensor(fpt, padded_indices(SITES, cap), GRID, BATCH, num_active=word(LIVE), status=status)

    def padded_go(y):                                  # zero in the dead rows, as the counted BatchNorm's backward leaves it
        g = np.zeros(tuple(y.features.shape), np.float32)
        g[:n_out] = go
        return dev(g)

    yp, *g_padded = run(x, padded_go)
    assert int(status) == 0 and yp.num_active.tolist() == [n_out] and yp.status is status
    assert torch.equal(yp.features[:n_out], y.features) and torch.equal(yp.indices[:n_out], y.indices)
    assert not yp.features[n_out:].any() and (yp.indices[n_out:] == -1).all()
    assert torch.equal(g_padded[0][:LIVE], g_compact[0]) and not g_padded[0][LIVE:].any()          # data gradient
    # float64 on the CPU: every product and partial sum is an integer below 2^24
    f64, w1d, b1d, w2d = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (f, w1, b1, w2))
    rows1, st1, _ = rs.conv_rows(f64, SITES, GRID, BATCH, w1d, b1d, 3, 1, 1, True)
    rows2, st2, _ = rs.conv_rows(rows1, st1, GRID, BATCH, w2d, None, 3, 2, 1, False)
    assert np.array_equal(st2, y.indices.cpu().numpy())
    ref = torch.autograd.grad(rows2, (f64, w1d, b1d, w2d), torch.tensor(go, dtype=torch.float64))
    assert max(float(t.abs().max()) for t in (rows1, rows2) + ref) < 2 ** 24
    assert np.array_equal(yp.features[:n_out].detach().cpu().numpy().astype(np.float64), rows2.detach().numpy())
    for what, a, c, r in zip(("g_feat", "g_w1", "g_b1", "g_w2"), g_padded, g_compact, ref):
        if what != "g_feat":
            assert torch.equal(a, c), what
            assert np.array_equal(a.cpu().numpy().astype(np.float64), r.numpy()), what
    assert np.array_equal(g_padded[0][:LIVE].cpu().numpy().astype(np.float64), ref[0].numpy())


# ---- backbones -----------------------------------------------------------------------------------------------------------------
def backbone_case(cls, seed, train):
    import test_second_net as t2
    coords, feats = t2.voxels(seed=seed)
    model = t2.make_backbone(cls, seed=5 if train else 1).train(train)
    gm = copy.deepcopy(model).cuda()
    with torch.no_grad():                                                   # the compact run gives the counts the caps come from
        out = copy.deepcopy(gm)({'voxel_features': dev(feats), 'voxel_coords': dev(coords), 'batch_size': t2.B})
    counts = {'spconv2': 'x_conv2', 'spconv3': 'x_conv3', 'spconv4': 'x_conv4'}
    counts = {k: out['multi_scale_3d_features'][v].features.shape[0] for k, v in counts.items()}
    counts['spconv_down2'] = out['encoded_spconv_tensor'].features.shape[0]
    gm.model_cfg = to_attr({'PADDED_CAPS': {k: (n + 63) // 64 * 64 + 64 for k, n in counts.items()}})
    cap = 1024
    fp = np.full((cap, feats.shape[1]), 7.0, np.float32)
    fp[:len(feats)] = feats
    batch = {'voxel_features': dev(fp), 'voxel_coords': padded_indices(coords, cap), 'batch_size': t2.B,
             'voxel_num_active': word(len(feats))}
    return t2, coords, feats, model, gm, batch, counts


@gpu
@pytest.mark.parametrize("name", ["VoxelBackBone8x", "VoxelResBackBone8x"])
def test_gpu_padded_backbone_train(name):
    from pdanet_amd import spconv_backbone
    t2, coords, feats, model, gm, batch, counts = backbone_case(getattr(spconv_backbone, name), 2, True)
    ref_m, ref_loss = t2.dense_train(model, feats, coords, torch.float64)
    f32_m, f32_loss = t2.dense_train(model, feats, coords, torch.float32)
    out = gm(batch)
    loss = (out['encoded_spconv_tensor'].features ** 2).sum()
    loss.backward()
    live, caps, status = sp.padded_report(out)
    assert status == 0 and live == dict(counts, input=len(feats)) and caps['input'] == 1024
    assert all(caps[k] == (n + 63) // 64 * 64 + 64 for k, n in counts.items())
    dev_fig = t2.figures(gm, float(loss.detach()), ref_m, ref_loss)
    f32_fig = t2.figures(f32_m, f32_loss, ref_m, ref_loss)
    for what, d, c in zip(("loss", "gradients", "running statistics"), dev_fig, f32_fig):
        print(name, "padded train", what, "device err", d, "float32 CPU err", c)
    for what, d, c in zip(("loss", "gradients", "running statistics"), dev_fig, f32_fig):
        assert d <= FACTOR * c, what
    assert all(int(v) == 1 for k, v in gm.named_buffers() if k.endswith('num_batches_tracked'))


@gpu
@pytest.mark.parametrize("name", ["VoxelBackBone8x", "VoxelResBackBone8x"])
def test_gpu_padded_backbone_eval(name):
    from pdanet_amd import spconv_backbone
    from pdanet_amd.height_compression import HeightCompression
    t2, coords, feats, model, gm, batch, counts = backbone_case(getattr(spconv_backbone, name), 0, False)
    with torch.no_grad():
        _, ref = t2.dense_outputs(model, feats, coords, torch.float64)
        _, f32 = t2.dense_outputs(model, feats, coords, torch.float32)
        out = HeightCompression(to_attr({'NUM_BEV_FEATURES': 256}))(gm(batch))
    r = ref['out'].values.numpy()
    bev = out['spatial_features'].cpu().numpy()
    assert bev.shape == (r.shape[0], r.shape[1] * r.shape[2]) + r.shape[3:]
    e_dev, e_f32 = t2.rel(bev.reshape(r.shape), r), t2.rel(f32['out'].values.numpy(), r)
    print(name, "padded eval BEV device err", e_dev, "float32 CPU err", e_f32)
    assert e_dev <= FACTOR * e_f32
    assert sp.padded_report(out)[2] == 0 and int(out['voxel_status']) == 0
    assert all(int(v) == 0 for k, v in gm.named_buffers() if k.endswith('num_batches_tracked'))


# ---- SECONDNet: no host read, graph replay -------------------------------------------------------------------------------------
def second_net_inputs():
    """The ragged pair of test_gpu_second_net_train_and_eval and a second pair with other counts, as generate_batch leaves them."""
    from pdanet_amd.voxel_utils import VoxelGenerator
    with open(os.path.join(HERE, "golden", "second_state_dict.json")) as f:
        cfg = json.load(f)['config']
    ds = cfg['dataset']
    pcr = np.array(ds['point_cloud_range'], np.float64)
    gen = VoxelGenerator(ds['voxel_size'], ds['point_cloud_range'], 4, 5, 2000)
    raw = []
    for seed, counts in ((5, [1500, 900]), (6, [700, 1300])):
        rng = np.random.default_rng(seed)
        pts = np.concatenate([np.concatenate([rng.uniform(pcr[:3], pcr[3:], (n, 3)), rng.random((n, 1))], axis=1) for n in counts])
        offs = torch.tensor([0, counts[0], sum(counts)], dtype=torch.int64).cuda()
        raw.append(gen.generate_batch((dev(pts.astype(np.float32)), offs, max(counts))))
    gt = np.zeros((2, 3, 8), np.float32)
    gt[0, 0] = [0.4, 0.0, -1.0, 3.9, 1.6, 1.56, 0.3, 1]
    gt[0, 1] = [0.3, 0.1, -0.6, 0.8, 0.6, 1.73, 1.2, 2]
    gt[1, 0] = [0.5, -0.1, -0.6, 1.76, 0.6, 1.73, -0.4, 3]
    return cfg, raw, dev(gt)


@gpu
def test_gpu_collate_padded_equals_collate():
    from pdanet_amd.voxel_utils import collate_voxels, collate_voxels_padded
    _, raw, _ = second_net_inputs()
    for voxels, coords, num_points, num_voxels in raw + [(raw[0][0], raw[0][1], raw[0][2], torch.tensor([-1, 5000], dtype=torch.int32).cuda())]:
        want = collate_voxels(voxels, coords, num_points, num_voxels)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            vox, crd, num, count, status = collate_voxels_padded(voxels, coords, num_points, num_voxels)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        n = want[0].shape[0]
        assert count.dtype == torch.int32 and count.tolist() == [n] and status.tolist() == [0] and status.dtype == torch.int32
        assert vox.shape == (2 * 2000, 5, 4) and crd.shape == (4000, 4) and num.shape == (4000,)
        assert torch.equal(vox[:n], want[0]) and torch.equal(crd[:n], want[1]) and torch.equal(num[:n], want[2])
        assert not vox[n:].any() and (crd[n:] == -1).all() and not num[n:].any()


@pytest.fixture
def deterministic_dense_kernels():
    """The dense 2D backbone and the head's convolutions run through MIOpen, whose default backward kernels add with float
    atomics: two eager runs on one input then differ in 60 of 61 tensors by ~1e-6 relative (measured on MI355X; the
    sparse part gives the same bits either way).  Bit-equality between eager and replay asks for its deterministic ones."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@gpu
def test_gpu_second_net_reads_nothing_and_replays_from_one_graph(deterministic_dense_kernels):
    from pdanet_amd.second_net import SECONDNet
    from pdanet_amd.voxel_utils import collate_voxels_padded
    cfg, raw, gt = second_net_inputs()
    torch.manual_seed(3)
    model = SECONDNet(to_attr(cfg['MODEL']), 3, cfg['dataset']).cuda().train()
    params = [p for p in model.parameters()]
    inputs = [collate_voxels_padded(*r) for r in raw]
    assert inputs[0][3].tolist() != inputs[1][3].tolist()
    static = [t.clone() for t in inputs[0]]                                # the padded buffers every run reads
    keys = ('voxels', 'voxel_coords', 'voxel_num_points', 'voxel_num_active', 'voxel_status')

    def load(which):
        for s, t in zip(static, inputs[which]):
            s.copy_(t)

    def step():
        batch = dict(zip(keys, static), gt_boxes=gt, batch_size=2)
        ret, tb, disp = model(batch)
        return (ret['loss'].detach(),) + torch.autograd.grad(ret['loss'], params)

    step()                                                                  # uploads the anchor table
    torch.cuda.synchronize()
    eager = []
    for which in (0, 1):
        load(which)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        eager.append([t.detach().clone() for t in out])
        assert static[4].tolist() == [0] and torch.isfinite(out[0])
        del out
    assert not torch.equal(eager[0][0], eager[1][0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    model.dense_head.forward_ret_dict.clear()                               # nothing of an earlier iteration alive at the capture
    gc.collect()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for which in (0, 1):
        load(which)
        graph.replay()
        torch.cuda.synchronize()
        assert static[4].tolist() == [0], (which, static[3].tolist(), [t[3].tolist() + t[4].tolist() for t in inputs])
        names = ['loss'] + [k for k, _ in model.named_parameters()]
        differ = [(k, float((a - c).abs().max())) for k, a, c in zip(names, eager[which], captured) if not torch.equal(a, c)]
        print("input", which, "replay differs from eager in", len(differ), "of", len(names), "tensors", differ[:8])
        stale = bool(differ) and all(torch.equal(a, c) for a, c in zip(eager[1 - which], captured))
        assert not differ, (which, "the replay gave the OTHER input's result" if stale else "", differ[:8])
