"""The residual tail of SparseBasicBlock on the padded path as one counted kernel pair (csrc/bn_relu.hip
pda_bn_add_relu_fwd_counted / _bwd_counted, spconv_utils.counted_batch_norm_add_relu):
y = relu(bn(x) + identity) over the live rows.

CPU part: the two entries are exported and bound and refuse bad sizes and null pointers before any launch.
GPU part, at the four widths of VoxelResBackBone8x and the row counts around a block's step:
(a) the fused call gives the bits of the composed padded sequence -- counted_batch_norm(relu=False), `+`, ReLU -- in y, grad_x,
    grad_identity, grad_gamma, grad_beta, the running buffers and the status word (the library is built with
    -ffp-contract=off and the fused expression rounds where the composed one rounds);
(b) dead rows of y, grad_x and grad_identity are exact zeros although the dead rows of x, identity and grad_y hold 7.0;
(c) against relu(F.batch_norm(x[:n]) + identity[:n]) and its autograd in float64 on the CPU the device may be off by FACTOR
    times the error of the same statement in float32 on the CPU (the rule and the FACTOR of tests/test_sparse_padded.py;
    figures are max |a - ref| / max |ref|, both are printed).  Training mode over fewer than two rows has no torch statement
    (torch raises): there FLAG_FEW_ROWS is set and everything stays finite.
A VoxelResBackBone8x with PDA_RES_BN unset (fused) equals the same backbone under PDA_RES_BN=composed bit for bit: the
features of all levels, the loss and every parameter gradient."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pdanet_amd import _lib, build, spconv_utils as sp

import test_sparse_padded as tsp
from test_sparse_padded import EPS, FACTOR, MOMENTUM, dev, rel, word

gpu = pytest.mark.gpu
ENTRIES = ["pda_bn_add_relu_fwd_counted", "pda_bn_add_relu_bwd_counted"]
CAP = 1024
NAMES = ("y", "grad_x", "grad_identity", "grad_gamma", "grad_beta", "running_mean", "running_var")


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_entries_are_exported_and_bound(lib):
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert callable(sp.counted_batch_norm_add_relu)


def test_argument_validation_without_gpu(lib):
    i64, f = ctypes.c_int64, ctypes.c_float
    words = (ctypes.c_int32 * 64)()
    buf = ctypes.addressof(words)          # 16-byte alignment is not promised: the size checks come first
    err = lib.pda_last_error
    fwd, bwd = lib.pda_bn_add_relu_fwd_counted, lib.pda_bn_add_relu_bwd_counted
    fwd_sizes = lambda cap, c: (i64(cap), c, f(1e-3), f(0.01))
    # null pointers
    assert fwd(*[None] * 9, *fwd_sizes(8, 16), None, None, 1, None) == 1 and b"null" in err()
    assert bwd(*[None] * 11, i64(8), 16, None, 1, None) == 1 and b"null" in err()
    for missing in range(9):               # every pointer but the running pair, which may be absent in training mode
        if missing in (4, 5):
            continue
        ptrs = [buf] * 9
        ptrs[missing] = None
        assert fwd(*ptrs, *fwd_sizes(8, 16), buf, buf, 1, None) == 1 and b"null" in err(), missing
    assert fwd(*[buf] * 9, *fwd_sizes(8, 16), None, buf, 1, None) == 1 and b"null" in err()
    assert fwd(*[buf] * 9, *fwd_sizes(8, 16), buf, None, 1, None) == 1 and b"null" in err()
    for missing in range(11):
        ptrs = [buf] * 11
        ptrs[missing] = None
        assert bwd(*ptrs, i64(8), 16, buf, 1, None) == 1 and b"null" in err(), missing
    assert bwd(*[buf] * 11, i64(8), 16, None, 1, None) == 1 and b"null" in err()
    # C out of range
    for c in (0, 2, 24, 2048):
        assert fwd(*[buf] * 9, *fwd_sizes(8, c), buf, buf, 1, None) == 1 and b"C = " in err()
        assert bwd(*[buf] * 11, i64(8), c, buf, 1, None) == 1 and b"C = " in err()
    # cap < 0
    assert fwd(*[buf] * 9, *fwd_sizes(-1, 16), buf, buf, 1, None) == 1 and b"bad size" in err()
    assert bwd(*[buf] * 11, i64(-1), 16, buf, 1, None) == 1 and b"bad size" in err()
    # one of the running pair alone; eval mode without them
    assert fwd(buf, buf, buf, buf, buf, None, buf, buf, buf, *fwd_sizes(8, 16), buf, buf, 1, None) == 1 and b"running" in err()
    assert fwd(buf, buf, buf, buf, None, None, buf, buf, buf, *fwd_sizes(8, 16), buf, buf, 0, None) == 1 and b"running" in err()


def test_an_empty_capacity_is_ok(lib):
    """cap == 0 returns PDA_OK; the forward touches nothing (the backward's two C-float gradients are zeroed by a device call,
    so it is in the GPU part)."""
    i64, f = ctypes.c_int64, ctypes.c_float
    keep = (ctypes.c_int32 * 64)()
    buf = (ctypes.addressof(keep) + 15) // 16 * 16          # the pointer checks come before the empty return
    assert lib.pda_bn_add_relu_fwd_counted(*[buf] * 9, i64(0), 16, f(1e-3), f(0.01), buf, buf, 1, None) == 0
    assert not any(keep)


def test_python_refuses_cpu_tensors():
    bn = torch.nn.BatchNorm1d(16)
    one = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sp.counted_batch_norm_add_relu(bn, torch.zeros(8, 16), torch.zeros(8, 16), one, one)


def test_the_switch_takes_two_values(monkeypatch):
    """PDA_RES_BN is read when a block runs; anything but 'fused' and 'composed' raises."""
    from pdanet_amd.config import fused_or_composed
    monkeypatch.delenv("PDA_RES_BN", raising=False)
    assert fused_or_composed("PDA_RES_BN") == "fused"
    monkeypatch.setenv("PDA_RES_BN", "composed")
    assert fused_or_composed("PDA_RES_BN") == "composed"
    monkeypatch.setenv("PDA_RES_BN", "1")
    with pytest.raises(ValueError, match="PDA_RES_BN"):
        fused_or_composed("PDA_RES_BN")


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def inputs(c, seed):
    rng = np.random.default_rng(seed)
    d = {'x': rng.standard_normal((CAP, c)) * 2 + 0.5, 'id': rng.standard_normal((CAP, c)), 'go': rng.standard_normal((CAP, c)),
         'w': rng.random(c) + 0.5, 'b': rng.standard_normal(c) * 0.3, 'rm': rng.standard_normal(c) * 0.1, 'rv': rng.random(c) + 0.5}
    return {k: v.astype(np.float32) for k, v in d.items()}


def statement(d, live, training, dtype):
    """relu(F.batch_norm(x[:live]) + identity[:live]) on the CPU with its autograd, in NAMES' order."""
    t = lambda k: torch.tensor(d[k], dtype=dtype)
    x, ident = t('x')[:live].requires_grad_(True), t('id')[:live].requires_grad_(True)
    w, b, rm, rv = t('w').requires_grad_(True), t('b').requires_grad_(True), t('rm'), t('rv')
    y = torch.relu(F.batch_norm(x, rm, rv, w, b, training, MOMENTUM, EPS) + ident)
    gx, gi, gw, gb = torch.autograd.grad(y, (x, ident, w, b), t('go')[:live])
    return [v.detach().numpy() for v in (y, gx, gi, gw, gb, rm, rv)]


def device(d, live, training, fused):
    """The fused call, or the composed padded sequence, with 7.0 in the dead rows of x, identity and grad_y: NAMES' tensors
    (on the device), the status word and num_batches_tracked."""
    c = d['x'].shape[1]
    bn = torch.nn.BatchNorm1d(c, eps=EPS, momentum=MOMENTUM).cuda().train(training)
    with torch.no_grad():
        bn.weight.copy_(dev(d['w'])), bn.bias.copy_(dev(d['b'])), bn.running_mean.copy_(dev(d['rm'])), bn.running_var.copy_(dev(d['rv']))
    x, ident, go = d['x'].copy(), d['id'].copy(), d['go'].copy()
    x[live:], ident[live:], go[live:] = 7.0, 7.0, 7.0
    x, ident = dev(x).requires_grad_(True), dev(ident).requires_grad_(True)
    count, status = word(live), word()
    if fused:
        y = sp.counted_batch_norm_add_relu(bn, x, ident, count, status)
    else:
        # the block's own sequence; its identity is another padded tensor's features, whose dead rows are zeros
        live_rows = (torch.arange(CAP, device='cuda') < live).unsqueeze(1)
        y = torch.relu(sp.counted_batch_norm(bn, x, count, status, relu=False) + torch.where(live_rows, ident, torch.zeros_like(ident)))
        go[live:] = 0.0                      # and its incoming gradient is zero there (the next counted kernel wrote it)
    gx, gi, gw, gb = torch.autograd.grad(y, (x, ident, bn.weight, bn.bias), dev(go))
    return [t.detach() for t in (y, gx, gi, gw, gb, bn.running_mean, bn.running_var)], int(status), int(bn.num_batches_tracked)


@gpu
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("c", [16, 32, 64, 128])
def test_gpu_bn_add_relu(c, training):
    rows_per_block = 1024 // c
    for live in (0, 1, 2, rows_per_block * 3 + 1, CAP):
        d = inputs(c, 2000 + c + live)
        got, status, tracked = device(d, live, training, fused=True)
        want, status_c, tracked_c = device(d, live, training, fused=False)
        # (a) the bits of the composed sequence
        assert status == status_c == (sp.FLAG_FEW_ROWS if training and live < 2 else 0), (live, status, status_c)
        assert tracked == tracked_c == (1 if training else 0)
        for what, a, b in zip(NAMES, got, want):
            assert a.shape == b.shape and torch.equal(a, b), (what, live, float((a - b).abs().max()))
        # (b) dead rows are exact zeros
        for what, a in zip(NAMES[:3], got):
            assert a.shape == (CAP, c) and not a[live:].any(), (what, live)
        assert all(bool(torch.isfinite(a).all()) for a in got), live
        host = [a.cpu().numpy() for a in got]
        if not training:
            assert np.array_equal(host[5], d['rm']) and np.array_equal(host[6], d['rv'])
        if live == 0:
            assert not host[3].any() and not host[4].any()
            assert np.array_equal(host[5], d['rm']) and np.array_equal(host[6], d['rv'])      # the running statistics stay
            continue
        if training and live < 2:
            continue                                                                          # torch raises: no statement
        # (c) against the float64 statement, within FACTOR times the float32 CPU error of the same statement
        ref, f32 = statement(d, live, training, torch.float64), statement(d, live, training, torch.float32)
        live_got = [a[:live] for a in host[:3]] + host[3:]
        for what, a, r, c32 in zip(NAMES, live_got, ref, f32):
            if not training and what.startswith("running"):
                continue
            e_dev, e_f32 = rel(a, r), rel(c32, r)
            print("bn add relu C=%d live=%d cap=%d training=%d %s device err %.3g float32 CPU err %.3g"
                  % (c, live, CAP, training, what, e_dev, e_f32))
            assert e_dev <= FACTOR * e_f32, (what, live, e_dev, e_f32)
        # the same bits from run to run
        again, _, _ = device(d, live, training, fused=True)
        for what, a, b in zip(NAMES, got, again):
            assert torch.equal(a, b), (what, live)


@gpu
def test_gpu_an_empty_capacity_backward_is_ok():
    """cap == 0 through the C entry: PDA_OK, grad_gamma and grad_beta zeroed, nothing else touched."""
    c = 16
    lib = _lib.load()
    t = torch.full((8, c), 3.0, device='cuda')
    gw, gb = torch.full((c,), 5.0, device='cuda'), torch.full((c,), 5.0, device='cuda')
    p, n = t.data_ptr(), word(0)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.pda_bn_add_relu_bwd_counted(p, p, p, p, p, p, p, p, gw.data_ptr(), gb.data_ptr(), p, ctypes.c_int64(0), c,
                                           n.data_ptr(), 1, stream) == 0
    torch.cuda.synchronize()
    assert not gw.any() and not gb.any() and bool((t == 3.0).all())


@gpu
def test_gpu_res_backbone_fused_equals_composed_bits(monkeypatch):
    """VoxelResBackBone8x on the padded input of tests/test_sparse_padded.py's backbone_case (grid 16 x 16 x 40, cap 1024, two
    scenes): the fused residual tails against PDA_RES_BN=composed."""
    from pdanet_amd.spconv_backbone import VoxelResBackBone8x
    _, coords, feats, _, gm, batch, _ = tsp.backbone_case(VoxelResBackBone8x, 2, True)
    runs = {}
    for mode in ("fused", "composed"):
        if mode == "fused":
            monkeypatch.delenv("PDA_RES_BN", raising=False)
        else:
            monkeypatch.setenv("PDA_RES_BN", mode)
        m = copy.deepcopy(gm).train()
        out = m(dict(batch))
        loss = (out['encoded_spconv_tensor'].features ** 2).sum()
        loss.backward()
        levels = dict(out['multi_scale_3d_features'], out=out['encoded_spconv_tensor'])
        assert sp.padded_report(out)[2] == 0
        runs[mode] = ({k: v.features.detach() for k, v in levels.items()}, loss.detach(),
                      {k: p.grad for k, p in m.named_parameters()}, {k: v for k, v in m.named_buffers()})
    monkeypatch.setenv("PDA_RES_BN", "both")
    with pytest.raises(ValueError, match="PDA_RES_BN"):
        copy.deepcopy(gm)(dict(batch))
    (f_lv, f_loss, f_grad, f_buf), (c_lv, c_loss, c_grad, c_buf) = runs["fused"], runs["composed"]
    assert set(f_lv) == {'x_conv1', 'x_conv2', 'x_conv3', 'x_conv4', 'out'}
    for k in f_lv:
        assert torch.equal(f_lv[k], c_lv[k]), k
    assert torch.isfinite(f_loss) and torch.equal(f_loss, c_loss)
    assert set(f_grad) == set(c_grad) and all(g is not None for g in f_grad.values())
    for k in f_grad:
        assert torch.equal(f_grad[k], c_grad[k]), k
    for k in f_buf:
        assert torch.equal(f_buf[k], c_buf[k]), k
