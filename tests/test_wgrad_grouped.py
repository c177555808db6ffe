"""First stages alone + one grouped second stage (pda_linear_wgrad_partials, pda_linear_wgrad_bn_partials,
pda_layer_norm_bwd_partials, pda_param_grad_reduce_grouped; include/pda_train.h) against the per-problem entries
pda_linear_wgrad / pda_linear_wgrad_bn / pda_layer_norm_bwd on the same inputs.  The grouped kernel runs each entry's
per-problem body unchanged, so every comparison is torch.equal: no tolerance anywhere in this file."""
import ctypes

import pytest
import torch

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from pdanet_amd import _lib
    return _lib.load()


# ---- CPU: argument validation (nothing here reaches a HIP call) ---------------------------------------------------------

def _entry(**kw):
    from pdanet_amd import _lib
    base = dict(kind=0, count=4, part=64, part_bias=None, dst=64, dst_bias=None, nm=32 * 12, n=32, cols=12, ld=12)
    base.update(kw)
    return _lib.ParamGradEntry(**base)


def test_grouped_call_validates_its_arguments(lib):
    from pdanet_amd import _lib
    one = (_lib.ParamGradEntry * 1)(_entry())
    assert lib.pda_param_grad_reduce_grouped(one, 0, None) == 1 and b"bad size" in lib.pda_last_error()
    assert lib.pda_param_grad_reduce_grouped(one, -3, None) == 1 and b"bad size" in lib.pda_last_error()
    assert lib.pda_param_grad_reduce_grouped(None, 0, None) == 1 and b"bad size" in lib.pda_last_error()       # the size first
    assert lib.pda_param_grad_reduce_grouped(None, 2, None) == 1 and b"null" in lib.pda_last_error()
    bad = [(dict(count=0), b"bad size"), (dict(count=-1), b"bad size"), (dict(kind=2), b"bad size"), (dict(n=0), b"bad size"),
           (dict(nm=32 * 12 + 1), b"bad size"), (dict(ld=11), b"bad size"), (dict(cols=0, nm=0), b"bad size"),
           (dict(kind=1, count=0, n=256, dst_bias=64), b"bad size"), (dict(kind=1, n=0, dst_bias=64), b"bad size"),
           (dict(count=0, part=None, dst=None), b"bad size"),                                                  # the size first
           (dict(part=None), b"null"), (dict(dst=None), b"null"), (dict(dst_bias=64), b"null"),               # bias without partials
           (dict(kind=1, n=256), b"null")]                                                                     # LayerNorm writes both
    for kw, what in bad:
        arr = (_lib.ParamGradEntry * 2)(_entry(), _entry(**kw))           # a bad entry behind a good one: nothing is launched
        assert lib.pda_param_grad_reduce_grouped(arr, 2, None) == 1, kw
        assert what in lib.pda_last_error(), (kw, lib.pda_last_error())


def test_first_stage_entries_validate_their_arguments(lib):
    i64, s = ctypes.c_int64, ctypes.c_int(0)
    p = ctypes.byref(s)
    for t, ni, no in [(0, 64, 64), (-1, 64, 64), (4096, 0, 64), (4096, 64, 6), (4096, 2, 64)]:
        assert lib.pda_linear_wgrad_partials(None, None, None, 1, i64(t), ni, no, None, None) == 1 and b"bad size" in lib.pda_last_error()
        assert lib.pda_linear_wgrad_bn_partials(None, None, None, i64(t), ni, no, None, None, None, None, None) == 1
        assert b"bad size" in lib.pda_last_error()
    assert lib.pda_linear_wgrad_partials(None, None, None, 1, i64(4096), 64, 64, None, None) == 1 and b"null" in lib.pda_last_error()
    assert lib.pda_linear_wgrad_partials(None, None, None, 1, i64(4096), 64, 64, p, None) == 1 and b"null" in lib.pda_last_error()
    assert lib.pda_linear_wgrad_bn_partials(None, None, None, i64(65536), 256, 256, None, None, None, p, None) == 1
    assert b"null" in lib.pda_last_error()
    assert lib.pda_linear_wgrad_bn_partials(None, None, None, i64(4096), 64, 64, None, None, None, p, None) != 0      # not the split form
    for rows, d in [(0, 256), (-5, 512), (100, 0), (100, 300)]:
        assert lib.pda_layer_norm_bwd_partials(None, None, None, 0, None, None, None, None, None, i64(rows), d, None, None) == 1
        assert b"bad size" in lib.pda_last_error()
    assert lib.pda_layer_norm_bwd_partials(None, None, None, 0, None, None, None, None, None, i64(33), 256, None, None) == 1
    assert b"null" in lib.pda_last_error()
    assert lib.pda_layer_norm_bwd_partials(None, None, None, 0, None, None, None, None, None, i64(33), 256, p, None) == 1
    assert b"null" in lib.pda_last_error()
    assert s.value == 0
    assert lib.pda_abi_version() == 20


def test_group_on_the_cpu_collects_nothing(lib):
    """Without a device tensor nothing is queued: a group that received no entry launches nothing, and one left by an
    exception drops what it held."""
    from pdanet_amd import pointnet2_batch_cuda as ext
    with ext.param_grad_group() as g:
        assert ext.param_grad_group_open() == ext.WGRAD_GROUPED
        with ext.param_grad_group() as inner:                  # joins the outer group
            assert ext._open_group() is (g if ext.WGRAD_GROUPED else None)
        assert not inner.entries
        with pytest.raises(RuntimeError):
            ext.linear_wgrad(torch.zeros(8, 4), torch.zeros(8, 4), torch.zeros(4, 4), None, 8, 4, 4)      # CPU tensors: refused
        assert not g.entries and not g.keep
    assert not ext.param_grad_group_open()
    with pytest.raises(ValueError):
        with ext.param_grad_group() as g:
            g.entries.append(object())
            raise ValueError("backward raised")
    assert not g.entries and not ext.param_grad_group_open()


# ---- GPU, native ------------------------------------------------------------------------------------------------------------

def _stream():
    return torch.cuda.current_stream().cuda_stream


def _wgrad_case(lib, tokens, n_in, n_out, bias, bn=False, seed=0):
    """Inputs, the per-problem entry's result (the reference, computed once) and the first stage's partials."""
    from pdanet_amd import _lib
    gen = torch.Generator(device="cuda").manual_seed(1000 + seed)
    x = torch.randn(tokens, n_in, device="cuda", generator=gen)
    g = torch.randn(tokens, n_out, device="cuda", generator=gen)
    nbytes = int(lib.pda_linear_wgrad_scratch_bytes(tokens, n_in, n_out))
    gw = torch.full((n_out, n_in), float("nan"), device="cuda")
    gb = torch.full((n_out,), float("nan"), device="cuda") if bias else None
    scratch0 = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    part = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    s = ctypes.c_int(0)
    if bn:
        mi = torch.cat([torch.randn(n_in, device="cuda", generator=gen) * 0.1, torch.rand(n_in, device="cuda", generator=gen) + 0.5])
        ga, be = torch.rand(n_in, device="cuda", generator=gen) + 0.5, torch.randn(n_in, device="cuda", generator=gen) * 0.1
        _lib.check(lib.pda_linear_wgrad_bn(x.data_ptr(), g.data_ptr(), gw.data_ptr(), None, scratch0.data_ptr(), tokens, n_in, n_out,
                                           mi.data_ptr(), ga.data_ptr(), be.data_ptr(), _stream()), "pda_linear_wgrad_bn")
        _lib.check(lib.pda_linear_wgrad_bn_partials(x.data_ptr(), g.data_ptr(), part.data_ptr(), tokens, n_in, n_out, mi.data_ptr(),
                                                    ga.data_ptr(), be.data_ptr(), ctypes.byref(s), _stream()), "pda_linear_wgrad_bn_partials")
    else:
        _lib.check(lib.pda_linear_wgrad(x.data_ptr(), g.data_ptr(), gw.data_ptr(), None if gb is None else gb.data_ptr(),
                                        scratch0.data_ptr(), tokens, n_in, n_out, _stream()), "pda_linear_wgrad")
        _lib.check(lib.pda_linear_wgrad_partials(x.data_ptr(), g.data_ptr(), part.data_ptr(), int(bias), tokens, n_in, n_out,
                                                 ctypes.byref(s), _stream()), "pda_linear_wgrad_partials")
    assert s.value * (n_in * n_out + n_out) * 4 == nbytes
    return dict(part=part, S=s.value, n_in=n_in, n_out=n_out, bias=bias, gw=gw, gb=gb)


def _wgrad_entry(c, dst, dst_bias):
    from pdanet_amd import _lib
    nm = c["n_in"] * c["n_out"]
    p = c["part"].data_ptr()
    return _lib.ParamGradEntry(0, c["S"], p, p + 4 * c["S"] * nm if dst_bias is not None else None, dst.data_ptr(),
                               None if dst_bias is None else dst_bias.data_ptr(), nm, c["n_out"], c["n_in"], dst.stride(0))


def _reduce(lib, entries):
    from pdanet_amd import _lib
    arr = (_lib.ParamGradEntry * len(entries))(*entries)
    _lib.check(lib.pda_param_grad_reduce_grouped(arr, len(entries), _stream()), "pda_param_grad_reduce_grouped")


@gpu
@pytest.mark.parametrize("tokens,n_in,n_out,bias,bn,slices", [
    (5000, 12, 32, False, False, 9),          # skinny form, ragged last slice
    (700, 64, 64, True, False, 1),            # skinny form, one slice
    (4099, 128, 256, True, False, 43),        # f32-MFMA form
    (64, 256, 128, True, False, 1),           # f32-MFMA form, one slice
    (32768, 256, 256, True, False, 128),      # split-bf16 form at the smallest shape that takes it
    (32768, 256, 256, False, True, 128),      # the same through the BatchNorm operand path
])
def test_first_stage_plus_grouped_equals_the_entry(lib, tokens, n_in, n_out, bias, bn, slices):
    c = _wgrad_case(lib, tokens, n_in, n_out, bias, bn)
    assert c["S"] == slices
    dw = torch.full_like(c["gw"], float("nan"))
    db = torch.full_like(c["gb"], float("nan")) if bias else None
    _reduce(lib, [_wgrad_entry(c, dw, db)])
    assert torch.equal(dw, c["gw"]) and not torch.isnan(dw).any()
    if bias:
        assert torch.equal(db, c["gb"]) and not torch.isnan(db).any()


@gpu
@pytest.mark.parametrize("tokens,n_in,n_out", [(4099, 128, 256), (5000, 12, 32), (4099, 36, 20)])
def test_both_load_widths_give_the_same_bits(lib, tokens, n_in, n_out):
    """The second stage reads 16 bytes per lane where sizes and alignment allow and 4 bytes otherwise, with the same
    additions in the same order: a copy of the partials 4 bytes off alignment (the 4-byte body) against the entry."""
    c = _wgrad_case(lib, tokens, n_in, n_out, True, seed=9)
    floats = c["part"].numel() // 4
    buf = torch.empty(floats + 4, device="cuda")
    shifted = buf[1:1 + floats]
    shifted.copy_(c["part"].view(torch.float32))
    assert shifted.data_ptr() % 16 == 4
    dw, db = torch.full_like(c["gw"], float("nan")), torch.full_like(c["gb"], float("nan"))
    _reduce(lib, [_wgrad_entry(dict(c, part=shifted), dw, db)])
    assert torch.equal(dw, c["gw"]) and torch.equal(db, c["gb"])


def _ln_case(lib, rows, d, two, seed=0):
    from pdanet_amd import _lib, pointnet2_batch_cuda as ext
    gen = torch.Generator(device="cuda").manual_seed(2000 + seed)
    x = torch.randn(rows, d, device="cuda", generator=gen)
    gy = torch.randn(rows, d, device="cuda", generator=gen)
    gy2 = torch.randn(rows, d, device="cuda", generator=gen) if two else None
    gamma = torch.rand(d, device="cuda", generator=gen) + 0.5
    st = torch.stack([x.mean(1), 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)], 1).contiguous()
    nbytes = ext.layer_norm_scratch_bytes(d)
    gx0, gg0, gb0 = torch.empty_like(x), torch.empty(d, device="cuda"), torch.empty(d, device="cuda")
    scratch0 = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(lib.pda_layer_norm_bwd(x.data_ptr(), gy.data_ptr(), None if gy2 is None else gy2.data_ptr(), gamma.data_ptr(), st.data_ptr(),
                                      gx0.data_ptr(), gg0.data_ptr(), gb0.data_ptr(), scratch0.data_ptr(), rows, d, _stream()), "pda_layer_norm_bwd")
    gx1 = torch.empty_like(x)
    part = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    nb = ctypes.c_int(0)
    _lib.check(lib.pda_layer_norm_bwd_partials(x.data_ptr(), gy.data_ptr(), None if gy2 is None else gy2.data_ptr(), 0, gamma.data_ptr(),
                                               st.data_ptr(), gx1.data_ptr(), None, part.data_ptr(), rows, d, ctypes.byref(nb), _stream()),
               "pda_layer_norm_bwd_partials")
    assert nb.value == min(1024, (rows + 3) // 4)
    assert torch.equal(gx0, gx1)
    return dict(part=part, nblocks=nb.value, d=d, gg=gg0, gb=gb0)


def _ln_entry(c, dgamma, dbeta):
    from pdanet_amd import _lib
    return _lib.ParamGradEntry(1, c["nblocks"], c["part"].data_ptr(), None, dgamma.data_ptr(), dbeta.data_ptr(), 0, c["d"], 0, 0)


@gpu
@pytest.mark.parametrize("rows", [33, 5000])
@pytest.mark.parametrize("d", [256, 512])
@pytest.mark.parametrize("two", [False, True])
def test_layer_norm_first_stage_plus_grouped_equals_the_entry(lib, rows, d, two):
    c = _ln_case(lib, rows, d, two)
    gg, gb = torch.full((d,), float("nan"), device="cuda"), torch.full((d,), float("nan"), device="cuda")
    _reduce(lib, [_ln_entry(c, gg, gb)])
    assert torch.equal(gg, c["gg"]) and torch.equal(gb, c["gb"]) and not torch.isnan(gg).any() and not torch.isnan(gb).any()


@pytest.fixture(scope="module")
def mixed(lib):
    """70 entries over seven problems (each reduced once by its own entry: the twins), with destinations of their own:
    more than one launch's worth (48 entries per launch), bias and no bias, nm = 720 (not a multiple of 64), LayerNorm
    entries in between and column-block destinations (row stride in + 3)."""
    cases = [_wgrad_case(lib, 5000, 12, 32, False, seed=1), _wgrad_case(lib, 700, 64, 64, True, seed=2),
             _wgrad_case(lib, 4099, 128, 256, True, seed=3), _wgrad_case(lib, 4099, 36, 20, True, seed=4),
             _wgrad_case(lib, 4099, 36, 20, False, seed=5)]
    lns = [_ln_case(lib, 5000, 256, True, seed=6), _ln_case(lib, 33, 512, False, seed=7)]
    entries, checks = [], []
    for i in range(70):
        k = i % 7
        if k >= 5:
            c = lns[k - 5]
            gg, gb = torch.full((c["d"],), float("nan"), device="cuda"), torch.full((c["d"],), float("nan"), device="cuda")
            entries.append(_ln_entry(c, gg, gb))
            checks.append((gg, c["gg"], gb, c["gb"], None))
            continue
        c = cases[k]
        strided = i % 3 == 0
        wide = torch.full((c["n_out"], c["n_in"] + 3), -7.0, device="cuda")
        dw = wide[:, 3:] if strided else torch.full((c["n_out"], c["n_in"]), float("nan"), device="cuda")
        db = torch.full((c["n_out"],), float("nan"), device="cuda") if c["bias"] else None
        entries.append(_wgrad_entry(c, dw, db))
        checks.append((dw, c["gw"], db, c["gb"], wide if strided else None))
    return entries, checks, cases + lns            # the entries hold raw pointers into the partials: keep those alive


def _check_mixed(checks):
    for dw, gw, db, gb, wide in checks:
        assert torch.equal(dw, gw)
        if db is not None:
            assert torch.equal(db, gb)
        if wide is not None:
            assert (wide[:, :3] == -7.0).all()          # the columns beside the block are not touched


@gpu
def test_seventy_mixed_entries_in_one_call(lib, mixed):
    entries, checks, _alive = mixed
    assert len(entries) == 70 and sum(1 for c in checks if c[4] is not None) >= 10
    _reduce(lib, entries)
    _check_mixed(checks)


@gpu
def test_grouped_call_captured_and_replayed(lib, mixed):
    entries, checks, _alive = mixed
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        _reduce(lib, entries)
    for _ in range(2):
        for dw, _gw, db, _gb, wide in checks:
            dw.fill_(float("nan"))
            if db is not None:
                db.fill_(float("nan"))
        graph.replay()
        _check_mixed(checks)
    torch.cuda.synchronize()


# ---- GPU, Python: one grouped launch per backward of a node that forms several parameter gradients ---------------------

def _block_grads(grouped, monkeypatch):
    """Gradients of a TransformerBlock (four weight gradients, two LayerNorms) and a LinearLongTokens + LayerNormResidual
    stand-in behind it, with the grouping switched on or off."""
    from pdanet_amd import pointnet2_batch_cuda as ext, pointnet2_utils as pu
    monkeypatch.setattr(ext, "WGRAD_GROUPED", grouped)
    torch.manual_seed(5)
    G, S, D, heads = 300, 16, 256, 4                         # 4800 tokens: above the kernels' 4096-token threshold
    layer = torch.nn.TransformerEncoderLayer(D, heads, dim_feedforward=512, dropout=0.0, norm_first=True).cuda()
    lin = torch.nn.Linear(D, D).cuda()
    ln = torch.nn.LayerNorm(D).cuda()
    x = torch.randn(G, S, D, device="cuda", requires_grad=True)
    assert pu.TransformerBlock.supported(x, heads)
    before = dict(ext.GROUP_STATS)
    y = pu.transformer_block(layer, x, pool=False)
    z = pu.layer_norm(pu.linear(y, lin.weight, lin.bias), ln, residual=y)
    gen = torch.Generator(device="cuda").manual_seed(6)
    z.backward(torch.randn(z.shape, device="cuda", generator=gen))
    params = list(layer.parameters()) + list(lin.parameters()) + list(ln.parameters())
    grads = [x.grad] + [p.grad for p in params if p.grad is not None]
    return grads, {k: ext.GROUP_STATS[k] - before[k] for k in ("grouped_calls", "entries")}


@gpu
def test_block_gradients_are_bit_equal_with_the_switch_on_and_off(monkeypatch):
    on, stats_on = _block_grads(True, monkeypatch)
    off, stats_off = _block_grads(False, monkeypatch)
    assert stats_on == {"grouped_calls": 1, "entries": 6}        # the block: 4 weights + 2 LayerNorms in one launch
    assert stats_off == {"grouped_calls": 0, "entries": 0}
    assert len(on) == len(off) >= 15
    for a, b in zip(on, off):
        assert torch.equal(a, b) and torch.isfinite(a).all()
