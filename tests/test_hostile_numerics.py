"""Hostile-input numerics: the BatchNorm, LayerNorm and attention kernels on inputs where a subtly wrong implementation
stops passing -- channels far from zero mean, constant channels and rows, a single outlier, a variance far below eps, a dead
ReLU, softmax scores in the thousands -- against an fp64 statement of the same operation in plain torch ops on the same
f32 inputs.

Yardstick (`within_rule`): with e_k = max|kernel - fp64| and e_t = max|torch's own f32 op - fp64| on the same device and
inputs, e_k <= 3 * e_t + 4 * 2**-24 * max|fp64|.  No hand-picked constant, and never the code under test.

The CPU test at the top checks that every input profile leaves torch's own f32 operators well conditioned (finite error
against fp64, and a non-zero one wherever the answer is not exact by construction); it carries no `gpu` mark, every other
test does.

ReLU masks and max-pool winners are discontinuous: an element whose fp64 pre-activation (or top-2 gap) is within 1e-3 of
the switch may legitimately fall on the other side in f32, in any implementation.  Such elements get a zero incoming
gradient, so the gradient checks never depend on them (`_margin`)."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

gpu = pytest.mark.gpu
U32 = 2.0 ** -24            # f32 unit roundoff
EPS, MOM = 1e-5, 0.1
MOM32 = float(np.float32(MOM))      # the kernels take the momentum as a C float
_MARGIN = 1e-3


def within_rule(what, got, ref64, lib):
    """The one acceptance rule of this file.  got: the HIP kernel's result; ref64: the fp64 statement; lib: torch's own
    f32 operator on the same device and inputs (rounded to the kernel's output format where that is bf16).
    e_k = max|got - ref64|, e_t = max|lib - ref64|, scale = max|ref64|; passes iff everything is finite and
    e_k <= 3 * e_t + 4 * 2**-24 * scale.  The factor 3 is the rule of tests/test_gemm_split.py (e < 3 * e_lib + 1e-7);
    the floor is four f32 unit roundoffs of the quantity's scale.  Prints one line per quantity (pytest -s / -rP)."""
    ref64 = ref64.detach().double()
    got, lib = got.detach().double().reshape(ref64.shape), lib.detach().double().reshape(ref64.shape)
    assert torch.isfinite(ref64).all(), what + ": the fp64 reference is not finite"
    assert torch.isfinite(got).all(), what + ": the kernel's result is not finite"
    scale = ref64.abs().max().item() if ref64.numel() else 0.0
    e_k = (got - ref64).abs().max().item() if ref64.numel() else 0.0
    e_t = (lib - ref64).abs().max().item() if ref64.numel() else 0.0
    bar = 3.0 * e_t + 4.0 * U32 * scale
    print("HOSTILE %-58s e_k=%.3e e_t=%.3e scale=%.3e bar=%.3e ratio=%.2f"
          % (what, e_k, e_t, scale, bar, e_k / max(e_t, 1e-300) if e_k > 0 else 0.0))
    assert math.isfinite(e_t), what + ": torch's own operator is not finite"
    assert e_k <= bar, "%s: e_k = %.3e > 3 * e_t + 4 * 2^-24 * scale = %.3e (e_t = %.3e, scale = %.3e)" % (what, e_k, bar, e_t, scale)


def _margin(switch64):
    """1 where the fp64 value that decides a ReLU mask / max-pool winner is safely away from its switching point."""
    return (switch64.detach().abs() > _MARGIN).to(switch64.dtype)


# ------------------------------------------------------------------------------------------------ input profiles
BN_PROFILES = "abcdefg"


def bn_profiles(rows, c, seed):
    """(x (rows, c), gamma, beta, kinds) on the CPU in f32; channel ch carries profile BN_PROFILES[ch % 7]:
    a N(0,1) | b 30 + N(0,1) | c 1000 + N(0,1) | d the constant 3.25 | e N(0,1) with one row at 1e4 | f 1e-4 N(0,1)
    (variance far below eps) | g gamma = 0.5, beta = -10: dead ReLU in every row."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, c, generator=g)
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g) * 0.3
    kinds = [BN_PROFILES[ch % 7] for ch in range(c)]
    for ch, k in enumerate(kinds):
        if k == "b":
            x[:, ch] += 30.0
        elif k == "c":
            x[:, ch] += 1000.0
        elif k == "d":
            x[:, ch] = 3.25
        elif k == "e":
            x[rows // 3, ch] = 1e4
        elif k == "f":
            x[:, ch] *= 1e-4
        elif k == "g":
            gamma[ch], beta[ch] = 0.5, -10.0
    return x, gamma, beta, kinds


def _chan(kinds, k, device):
    return torch.tensor([i for i, kk in enumerate(kinds) if kk == k], dtype=torch.long, device=device)


LN_PROFILES = ("control", "offset1000", "constant", "outlier", "tiny")


def ln_profiles(rows, d, seed, residual):
    """(x, res or None, gamma, beta, kinds) on the CPU; row r carries LN_PROFILES[r % 5] (of x + res when res is given)."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(rows, d, generator=g)
    kinds = [LN_PROFILES[r % 5] for r in range(rows)]
    for r, k in enumerate(kinds):
        if k == "offset1000":
            s[r] += 1000.0
        elif k == "constant":
            s[r] = 3.25
        elif k == "outlier":
            s[r, (7 * r) % d] = 1e4
        elif k == "tiny":
            s[r] *= 1e-4
    gamma, beta = torch.randn(d, generator=g), torch.randn(d, generator=g)
    if not residual:
        return s, None, gamma, beta, kinds
    res = torch.randn(rows, d, generator=g) * 0.5
    for r, k in enumerate(kinds):
        if k == "constant":
            res[r] = 1.25
    x = s - res
    for r, k in enumerate(kinds):
        if k == "constant":
            x[r] = 2.0                  # 2.0 + 1.25: the sum is the constant 3.25 without rounding
    return x, res, gamma, beta, kinds


ATT_PROFILES = ("control", "x8", "x30", "same_keys", "one_hot", "minus3000")
ATT_SHAPES = [(8, 32, 4, 37), (16, 64, 4, 37), (32, 128, 2, 5)]          # (S, hd, heads, G)


def att_profiles(S, hd, heads, G, seed):
    """qkv (G, S, 3 * heads * hd) on the CPU, laid out [q | k | v] x heads x hd; group g carries ATT_PROFILES[g % 6]."""
    gen = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(G, S, 3, heads, hd, generator=gen) * 0.7)
    kinds = [ATT_PROFILES[g % 6] for g in range(G)]
    for g, k in enumerate(kinds):
        if k == "x8":
            qkv[g] *= 8.0 / 0.7
        elif k == "x30":
            qkv[g] *= 30.0 / 0.7
        elif k == "same_keys":
            qkv[g, :, 1] = qkv[g, 0:1, 1]                  # uniform softmax: out = the plain mean of V
        elif k == "one_hot":
            u = torch.randn(heads, hd, generator=gen)
            qkv[g, :, 0] = u + 0.05 * torch.randn(S, heads, hd, generator=gen)
            qkv[g, :, 1] *= 0.1 / 0.7
            qkv[g, (3 * g) % S, 1] = 20.0 * u / u.norm(dim=-1, keepdim=True)      # one key = 20 x the query direction
        elif k == "minus3000":
            cval = math.sqrt(3000.0 / math.sqrt(hd))       # hd * cval^2 / sqrt(hd) = 3000
            qkv[g, :, 1] = cval
            qkv[g, :, 0] = -cval                           # every score is -3000
    return qkv.reshape(G, S, 3 * heads * hd).contiguous(), kinds


# ------------------------------------------------------------------------------------------------ fp64 / torch-f32 twins
def _leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


def bn_relu_twin(x, gamma, beta, rm0, rv0, dtype):
    """relu(batch_norm(x)) over the rows of x (rows, C) with batch statistics.  float64: the statement in plain ops;
    float32: torch's own F.batch_norm(training=True) + relu.  Returns the leaves and a dict of results."""
    xl, gl, bl = _leaf(x, dtype), _leaf(gamma, dtype), _leaf(beta, dtype)
    n = x.shape[0]
    mean = xl.detach().mean(0)
    var = xl.detach().var(0, unbiased=False)
    invstd = (var + EPS).rsqrt()
    if dtype == torch.float64:
        m_, v_ = xl.mean(0), xl.var(0, unbiased=False)
        pre = (xl - m_) * (v_ + EPS).rsqrt() * gl + bl
        unb = var * (n / (n - 1.0)) if n > 1 else var
        rm = (1.0 - MOM32) * rm0.double() + MOM32 * mean
        rv = (1.0 - MOM32) * rv0.double() + MOM32 * unb
    else:
        rm, rv = rm0.detach().clone(), rv0.detach().clone()
        pre = F.batch_norm(xl, rm, rv, gl, bl, True, MOM, EPS)
    return (xl, gl, bl), dict(pre=pre, y=torch.relu(pre), mean_invstd=torch.cat([mean, invstd]), rm=rm, rv=rv)


def _first_max(y):
    """max over dim 1 of y (groups, ns, C) routed to the FIRST slot that attains it (the kernels' documented tie rule)."""
    m = y.max(dim=1, keepdim=True)[0]
    first = (y == m).to(torch.uint8).argmax(dim=1, keepdim=True)
    return y.gather(1, first).squeeze(1)


def attention_twin(qkv, heads, dtype):
    """Self-attention over the S tokens of every group.  float64: softmax(q k^T / sqrt(hd)) v in plain ops;
    float32: F.scaled_dot_product_attention on the math backend.  Returns leaf, out (G, S, D), lse (G, heads, S)."""
    G, S, D3 = qkv.shape
    hd = D3 // (3 * heads)
    leaf = _leaf(qkv, dtype)
    q, k, v = leaf.view(G, S, 3, heads, hd).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
    lse = torch.logsumexp(s.detach(), dim=-1)
    if dtype == torch.float64:
        o = torch.softmax(s, dim=-1) @ v
    else:
        from torch.nn.attention import SDPBackend, sdpa_kernel
        with sdpa_kernel(SDPBackend.MATH):
            o = F.scaled_dot_product_attention(q, k, v)
    return leaf, o.transpose(1, 2).reshape(G, S, heads * hd), lse


# ------------------------------------------------------------------------------------------------ CPU: conditioning
def _et(lib, ref64):
    return (lib.detach().double() - ref64.detach()).abs().max().item()


def test_profiles_keep_torchs_own_operators_well_conditioned():
    """Every profile, on the CPU: torch's f32 operator against fp64 has a finite error, and a non-zero one wherever the
    answer is not exact by construction (constant channel / row, dead ReLU).  Anything else is a degenerate profile."""
    for rows, c in [(4099, 64), (2, 8)]:
        x, gamma, beta, kinds = bn_profiles(rows, c, seed=rows + c)
        rm0, rv0 = torch.zeros(c), torch.ones(c)
        _, r64 = bn_relu_twin(x, gamma, beta, rm0, rv0, torch.float64)
        _, r32 = bn_relu_twin(x, gamma, beta, rm0, rv0, torch.float32)
        for k in BN_PROFILES:
            ch = _chan(kinds, k, "cpu")
            e = _et(r32["y"][:, ch], r64["y"][:, ch])
            assert math.isfinite(e), (rows, k)
            if k not in "dg" and rows > 2:
                assert e > 0.0, (rows, k)
        for q in ("y", "rm", "rv"):
            e = _et(r32[q], r64[q])
            assert math.isfinite(e) and e > 0.0, (rows, q)
    for d in (256, 512, 1024):
        for residual in (False, True):
            x, res, gamma, beta, kinds = ln_profiles(77, d, seed=d, residual=residual)
            s = x if res is None else x + res
            y64 = F.layer_norm(s.double(), (d,), gamma.double(), beta.double(), EPS)
            y32 = F.layer_norm(s, (d,), gamma, beta, EPS)
            for k in LN_PROFILES:
                rws = torch.tensor([r for r, kk in enumerate(kinds) if kk == k], dtype=torch.long)
                e = _et(y32[rws], y64[rws])
                assert math.isfinite(e), (d, k)
                if k != "constant":
                    assert e > 0.0, (d, k)
                else:
                    assert torch.equal(y64[rws], beta.double().expand(len(rws), d))
    for S, hd, heads, G in ATT_SHAPES:
        qkv, kinds = att_profiles(S, hd, heads, G, seed=S + hd)
        _, o64, l64 = attention_twin(qkv, heads, torch.float64)
        _, o32, l32 = attention_twin(qkv, heads, torch.float32)
        assert torch.isfinite(o64).all() and torch.isfinite(l64).all()
        for k in ATT_PROFILES:
            gs = torch.tensor([g for g, kk in enumerate(kinds) if kk == k], dtype=torch.long)
            if gs.numel() == 0:
                continue                    # G = 5 ends before the last profile
            e = _et(o32[gs], o64[gs])
            assert math.isfinite(e) and e > 0.0, (S, k)
            if k == "minus3000":
                assert (l64[gs] - (math.log(S) - 3000.0)).abs().max().item() < 1e-2        # the profile is what it says


def test_rule_rejects_known_wrong_variants():
    """The bar has teeth: f32 twins that are wrong in the ways this file is about miss it, on the CPU."""
    x, gamma, beta, kinds = bn_profiles(4099, 64, seed=4163)
    rm0, rv0 = torch.zeros(64), torch.ones(64)
    _, r64 = bn_relu_twin(x, gamma, beta, rm0, rv0, torch.float64)
    _, r32 = bn_relu_twin(x, gamma, beta, rm0, rv0, torch.float32)
    mean = x.sum(0) / x.shape[0]                                    # one-pass f32 statistics: E[x^2] - mean^2
    var = ((x * x).sum(0) / x.shape[0] - mean * mean).clamp_min(0)
    y_wrong = torch.relu((x - mean) * (var + EPS).rsqrt() * gamma + beta)
    with pytest.raises(AssertionError, match="e_k"):
        within_rule("one-pass f32 BatchNorm statistics", y_wrong, r64["y"], r32["y"])
    qkv, _ = att_profiles(16, 64, 4, 37, seed=80)
    _, o64, _ = attention_twin(qkv, 4, torch.float64)
    _, o32, _ = attention_twin(qkv, 4, torch.float32)
    q, k, v = qkv.view(37, 16, 3, 4, 64).permute(2, 0, 3, 1, 4)
    p = torch.exp(q @ k.transpose(-1, -2) / 8.0)                    # softmax without the max subtraction
    o_wrong = ((p / p.sum(-1, keepdim=True)) @ v).transpose(1, 2).reshape(37, 16, 256)
    with pytest.raises(AssertionError):
        within_rule("softmax without max subtraction", o_wrong, o64, o32)


# ------------------------------------------------------------------------------------------------ BatchNorm family
def _bn_module(c, gamma, beta):
    bn = torch.nn.BatchNorm1d(c, eps=EPS, momentum=MOM).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    return bn


def _exact_checks(tag, kinds, y, dx, dgamma, dbeta, rv, beta, rows, first_only=None):
    """Profile d: y == relu(beta) bit for bit, dgamma == 0, dx finite, running_var exactly the fp64 value for a zero
    variance.  Profile g: y, dx, dgamma, dbeta all exactly zero."""
    dev = y.device
    d, g = _chan(kinds, "d", dev), _chan(kinds, "g", dev)
    y2 = y.reshape(-1, y.shape[-1])
    if d.numel():
        assert torch.equal(y2[:, d], torch.relu(beta[d]).expand(y2.shape[0], -1)), tag + ": constant channel, y != relu(beta)"
        assert torch.equal(dgamma[d], torch.zeros_like(dgamma[d])), tag + ": constant channel, dgamma != 0"
        assert torch.isfinite(dx.reshape(-1, dx.shape[-1])[:, d].float()).all(), tag
        if rv is not None:
            want = torch.tensor((1.0 - MOM32) * 1.0 + MOM32 * 0.0, dtype=torch.float64).float().item()
            assert torch.equal(rv[d], torch.full_like(rv[d], want)), tag + ": constant channel, running_var"
    if g.numel():
        assert not y2[:, g].any(), tag + ": dead channel, y != 0"
        assert not dx.reshape(-1, dx.shape[-1])[:, g].float().any(), tag + ": dead channel, dx != 0"
        assert not dgamma[g].any() and not dbeta[g].any(), tag + ": dead channel, dgamma / dbeta != 0"


@gpu
@pytest.mark.parametrize("rows,c", [(4099, 64), (2, 8)])
def test_bn_relu_plain(rows, c):
    from pdanet_amd import pointnet2_utils as pu
    x, gamma, beta, kinds = (t.cuda() if torch.is_tensor(t) else t for t in bn_profiles(rows, c, seed=rows + c))
    rm0, rv0 = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    l64, r64 = bn_relu_twin(x, gamma, beta, rm0, rv0, torch.float64)
    l32, r32 = bn_relu_twin(x, gamma, beta, rm0, rv0, torch.float32)
    gy = torch.randn(rows, c, device="cuda", generator=torch.Generator("cuda").manual_seed(1)) * _margin(r64["pre"]).float()
    bn = _bn_module(c, gamma, beta)
    xk = x.clone().requires_grad_(True)
    y = pu.batch_norm_relu(bn, xk)
    gk = torch.autograd.grad(y, (xk, bn.weight, bn.bias), gy)
    g64 = torch.autograd.grad(r64["y"], l64, gy.double())
    g32 = torch.autograd.grad(r32["y"], l32, gy)
    tag = "bn_relu plain %dx%d " % (rows, c)
    within_rule(tag + "y", y, r64["y"], r32["y"])
    within_rule(tag + "running_mean", bn.running_mean, r64["rm"], r32["rm"])
    within_rule(tag + "running_var", bn.running_var, r64["rv"], r32["rv"])
    for n, a, b, t in zip(("dx", "dgamma", "dbeta"), gk, g64, g32):
        within_rule(tag + n, a, b, t)
    _exact_checks(tag, kinds, y.detach(), gk[0], gk[1], gk[2], bn.running_var, beta, rows)


@gpu
def test_bn_relu_single_row():
    """rows = 1: torch refuses ("Expected more than 1 value per channel when training").  The kernel keeps the
    behaviour bn_finalize_fwd_kernel documents: the batch variance is 0, the unbiased variance takes the rows > 1 guard
    and is 0 too, so y == relu(beta), dx == 0, dgamma == 0, dbeta == the masked grad_y, running_mean moves to x and
    running_var to (1 - momentum) * running_var -- all exact."""
    from pdanet_amd import pointnet2_utils as pu
    x, gamma, beta, kinds = (t.cuda() if torch.is_tensor(t) else t for t in bn_profiles(1, 8, seed=9))
    with pytest.raises(ValueError, match="more than 1 value"):
        F.batch_norm(x, torch.zeros(8, device="cuda"), torch.ones(8, device="cuda"), gamma, beta, True, MOM, EPS)
    bn = _bn_module(8, gamma, beta)
    xk = x.clone().requires_grad_(True)
    y = pu.batch_norm_relu(bn, xk)
    gy = torch.randn(1, 8, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    dx, dg, db = torch.autograd.grad(y, (xk, bn.weight, bn.bias), gy)
    assert torch.equal(y.detach(), torch.relu(beta).view(1, 8))
    assert not dx.any() and not dg.any()
    assert torch.equal(db, (gy * (beta > 0)).view(8))
    assert torch.equal(bn.running_mean, (MOM32 * x.double().view(8)).float())
    assert torch.equal(bn.running_var, torch.full((8,), 1.0 - MOM32, dtype=torch.float64).float().cuda())


@gpu
def test_bn_relu_bf16_boundary():
    """ext.bn_relu_fwd / bwd with bf16 x and grad_y: inputs rounded to bf16 first, fp64 on the rounded values; the bf16
    grad_x is compared with torch's f32 result rounded to bf16."""
    from pdanet_amd import pointnet2_batch_cuda as ext
    rows, c = 4099, 64
    x, gamma, beta, kinds = (t.cuda() if torch.is_tensor(t) else t for t in bn_profiles(rows, c, seed=77))
    xb = x.bfloat16()
    rm0, rv0 = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    l64, r64 = bn_relu_twin(xb.float(), gamma, beta, rm0, rv0, torch.float64)
    l32, r32 = bn_relu_twin(xb.float(), gamma, beta, rm0, rv0, torch.float32)
    gyb = (torch.randn(rows, c, device="cuda", generator=torch.Generator("cuda").manual_seed(3)) * _margin(r64["pre"]).float()).bfloat16()
    scratch = torch.empty(ext.bn_relu_scratch_bytes(c), dtype=torch.uint8, device="cuda")
    rm, rv = rm0.clone(), rv0.clone()
    y, st = torch.empty(rows, c, device="cuda"), torch.empty(2, c, device="cuda")
    ext.bn_relu_fwd(xb, gamma, beta, rm, rv, y, st, scratch, rows, c, EPS, MOM)
    gx, gg, gb = torch.empty_like(xb), torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    ext.bn_relu_bwd(xb, gyb, gamma, beta, st, gx, gg, gb, scratch, rows, c)
    g64 = torch.autograd.grad(r64["y"], l64, gyb.double())
    g32 = torch.autograd.grad(r32["y"], l32, gyb.float())
    tag = "bn_relu bf16 4099x64 "
    within_rule(tag + "y", y, r64["y"], r32["y"])
    within_rule(tag + "mean_invstd", st, r64["mean_invstd"], r32["mean_invstd"])
    within_rule(tag + "running_mean", rm, r64["rm"], r32["rm"])
    within_rule(tag + "running_var", rv, r64["rv"], r32["rv"])
    assert gx.dtype == torch.bfloat16
    within_rule(tag + "dx(bf16)", gx, g64[0], g32[0].bfloat16())
    within_rule(tag + "dgamma", gg, g64[1], g32[1])
    within_rule(tag + "dbeta", gb, g64[2], g32[2])
    _exact_checks(tag, kinds, y, gx, gg, gb, rv, beta, rows)


@gpu
def test_bn_relu_max_pool():
    from pdanet_amd import pointnet2_utils as pu
    shape = (2, 65, 16, 64)
    B, M, ns, c = shape
    x, gamma, beta, kinds = (t.cuda() if torch.is_tensor(t) else t for t in bn_profiles(B * M * ns, c, seed=65))
    rm0, rv0 = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    l64, r64 = bn_relu_twin(x, gamma, beta, rm0, rv0, torch.float64)
    l32, r32 = bn_relu_twin(x, gamma, beta, rm0, rv0, torch.float32)
    o64, o32 = _first_max(r64["y"].view(B * M, ns, c)), _first_max(r32["y"].view(B * M, ns, c))
    # winners decided by less than the margin (but not exact ties, which go to the first slot everywhere) get no gradient
    top = r64["y"].detach().view(B * M, ns, c).topk(2, dim=1)[0]
    gap = top[:, 0] - top[:, 1]
    safe = ((gap == 0) | (gap > _MARGIN)) & (r64["pre"].detach().view(B * M, ns, c).max(dim=1)[0].abs() > _MARGIN)
    go = torch.randn(B * M, c, device="cuda", generator=torch.Generator("cuda").manual_seed(4)) * safe.float()
    bn = torch.nn.BatchNorm2d(c, eps=EPS, momentum=MOM).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    xk = x.view(shape).clone().requires_grad_(True)
    assert pu.BatchNormReLUMaxPool.supported(xk, bn)
    out = pu.batch_norm_relu_max_pool(bn, xk)
    gk = torch.autograd.grad(out, (xk, bn.weight, bn.bias), go.view(B, M, c))
    g64 = torch.autograd.grad(o64, l64, go.double())
    g32 = torch.autograd.grad(o32, l32, go)
    tag = "bn_relu_max_pool (2,65,16,64) "
    within_rule(tag + "out", out, o64, o32)
    within_rule(tag + "running_mean", bn.running_mean, r64["rm"], r32["rm"])
    within_rule(tag + "running_var", bn.running_var, r64["rv"], r32["rv"])
    for n, a, b, t in zip(("dx", "dgamma", "dbeta"), gk, g64, g32):
        within_rule(tag + n, a, b, t)
    _exact_checks(tag, kinds, out.detach().view(B * M, c), gk[0], gk[1], gk[2], bn.running_var, beta, B * M * ns)


@gpu
def test_bn_relu_weighted():
    """pda_bn_relu_{fwd,bwd}_weighted through BatchNormReLUWeighted: 300 unique rows standing for 1..16 copies each, against
    dense BatchNorm of the expanded rows (a row's incoming gradient is the total over its copies)."""
    from pdanet_amd import pointnet2_utils as pu
    U, c = 300, 64
    x, gamma, beta, kinds = (t.cuda() if torch.is_tensor(t) else t for t in bn_profiles(U, c, seed=300))
    gen = torch.Generator("cuda").manual_seed(5)
    wts = torch.randint(1, 17, (U,), device="cuda", generator=gen)
    count = int(wts.sum())
    owner = torch.repeat_interleave(torch.arange(U, device="cuda"), wts)
    first = torch.cumsum(wts, 0) - wts
    rm0, rv0 = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    l64, r64 = bn_relu_twin(x[owner], gamma, beta, rm0, rv0, torch.float64)
    l32, r32 = bn_relu_twin(x[owner], gamma, beta, rm0, rv0, torch.float32)
    gy = torch.randn(U, c, device="cuda", generator=gen) * _margin(r64["pre"][first]).float()
    gy_dense = torch.zeros(count, c, device="cuda").index_copy_(0, first, gy)
    bn = _bn_module(c, gamma, beta)
    xk = x.clone().requires_grad_(True)
    y = pu.BatchNormReLUWeighted.apply(xk, bn.weight, bn.bias, bn.running_mean, bn.running_var, EPS, MOM, wts.float(), count)
    gk = torch.autograd.grad(y, (xk, bn.weight, bn.bias), gy)
    g64 = list(torch.autograd.grad(r64["y"], l64, gy_dense.double()))
    g32 = list(torch.autograd.grad(r32["y"], l32, gy_dense))
    g64[0] = torch.zeros(U, c, dtype=torch.float64, device="cuda").index_add_(0, owner, g64[0])
    g32[0] = torch.zeros(U, c, device="cuda").index_add_(0, owner, g32[0])
    tag = "bn_relu weighted 300x64 "
    within_rule(tag + "y", y, r64["y"][first], r32["y"][first])
    within_rule(tag + "running_mean", bn.running_mean, r64["rm"], r32["rm"])
    within_rule(tag + "running_var", bn.running_var, r64["rv"], r32["rv"])
    for n, a, b, t in zip(("dx", "dgamma", "dbeta"), gk, g64, g32):
        within_rule(tag + n, a, b, t)
    _exact_checks(tag, kinds, y.detach(), gk[0], gk[1], gk[2], bn.running_var, beta, count)


@gpu
def test_bn_stats_only():
    from pdanet_amd import pointnet2_batch_cuda as ext
    rows, c = 4099, 64
    x, gamma, beta, kinds = (t.cuda() if torch.is_tensor(t) else t for t in bn_profiles(rows, c, seed=11))
    rm0, rv0 = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    _, r64 = bn_relu_twin(x, gamma, beta, rm0, rv0, torch.float64)
    _, r32 = bn_relu_twin(x, gamma, beta, rm0, rv0, torch.float32)
    rm, rv, st = rm0.clone(), rv0.clone(), torch.empty(2, c, device="cuda")
    scratch = torch.empty(ext.bn_relu_scratch_bytes(c), dtype=torch.uint8, device="cuda")
    ext.bn_stats_fwd(x, rm, rv, st, scratch, rows, c, EPS, MOM)
    tag = "bn_stats_fwd 4099x64 "
    within_rule(tag + "mean_invstd", st, r64["mean_invstd"], r32["mean_invstd"])
    within_rule(tag + "running_mean", rm, r64["rm"], r32["rm"])
    within_rule(tag + "running_var", rv, r64["rv"], r32["rv"])
    d = _chan(kinds, "d", "cuda")
    assert torch.equal(st[0, d], torch.full_like(st[0, d], 3.25))
    assert torch.equal(st[1, d], torch.full_like(st[1, d], float(torch.tensor(EPS, dtype=torch.float32).double().rsqrt().float())))


@gpu
def test_gemm_epilogue_statistics():
    """ext.gemm_split_bn(stats_mode=1) + pda_bn_finalize_fwd: the OUTPUT columns carry the profiles.  Input column 0 is the
    constant 1 and column 1 is zero except for a 1 in one row, so a weight row places the offset (w[:, 0]) and the outlier
    (w[:, 1]); the remaining columns are N(0, 1) and the weight row is scaled to give them unit (or 1e-4, or zero) spread."""
    from pdanet_amd import pointnet2_batch_cuda as ext
    T, K, N = 513, 32, 256
    gen = torch.Generator("cuda").manual_seed(6)
    x = torch.randn(T, K, device="cuda", generator=gen)
    x[:, 0] = 1.0
    x[:, 1] = 0.0
    x[T // 3, 1] = 1.0
    w = torch.randn(N, K, device="cuda", generator=gen)
    w[:, 2:] /= w[:, 2:].norm(dim=1, keepdim=True)
    w[:, :2] = 0.0
    kinds = [BN_PROFILES[n % 7] for n in range(N)]
    for n, k in enumerate(kinds):
        if k == "b":
            w[n, 0] = 30.0
        elif k == "c":
            w[n, 0] = 1000.0
        elif k == "d":
            w[n] = 0.0
            w[n, 0] = 3.25
        elif k == "e":
            w[n, 1] = 1e4
        elif k == "f":
            w[n] *= 1e-4
    z64 = x.double() @ w.double().t()
    z32 = x @ w.t()
    rm0, rv0 = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")
    one, zero = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
    _, r64 = bn_relu_twin(z64, one, zero, rm0, rv0, torch.float64)
    _, r32 = bn_relu_twin(z32, one, zero, rm0, rv0, torch.float32)
    wf = ext.linear_split_pack(w, N, K)
    tiles = ext.gemm_split_bn_tiles(T)
    y = torch.full((T, N), float("nan"), device="cuda")
    part = torch.full((tiles * 2 * N,), float("nan"), dtype=torch.float64, device="cuda")
    ext.gemm_split_bn(x, wf, y, T, K, N, stats_mode=1, partial=part)
    rm, rv, st = rm0.clone(), rv0.clone(), torch.empty(2 * N, device="cuda")
    ext.bn_finalize_fwd(part, tiles, N, T, EPS, MOM, st, rm, rv)
    tag = "gemm epilogue 513x32x256 "
    within_rule(tag + "z", y, z64, z32)
    within_rule(tag + "mean_invstd", st, r64["mean_invstd"], r32["mean_invstd"])
    within_rule(tag + "running_mean", rm, r64["rm"], r32["rm"])
    within_rule(tag + "running_var", rv, r64["rv"], r32["rv"])
    d = _chan(kinds, "d", "cuda")
    assert torch.equal(y[:, d], torch.full_like(y[:, d], 3.25))
    assert torch.equal(st[d], torch.full_like(st[d], 3.25))


def _smallest_split_wgrad_tokens(k, n):
    from pdanet_amd import _lib
    lib = _lib.load()
    for t in range(4096, 1 << 20, 4096):
        if int(lib.pda_linear_wgrad_form(t, k, n)) == 2:
            return t
    raise AssertionError("no split-form weight gradient below 2^20 tokens")


@gpu
def test_gemm_prologue_and_wgrad_with_bn_in_the_operand_load():
    """ext.gemm_split_bn(in_bn=...) and ext.linear_wgrad_bn at the smallest token count on the split weight-gradient form:
    the INPUT channels carry the profiles, their mean / invstd are given from fp64."""
    from pdanet_amd import pointnet2_batch_cuda as ext
    K = N = 256
    T = _smallest_split_wgrad_tokens(K, N)
    x, gamma, beta, kinds = (t.cuda() if torch.is_tensor(t) else t for t in bn_profiles(T, K, seed=256))
    gen = torch.Generator("cuda").manual_seed(7)
    w = torch.randn(N, K, device="cuda", generator=gen) * 0.05
    gz = torch.randn(T, N, device="cuda", generator=gen)
    x64 = x.double()
    mi = torch.cat([x64.mean(0), (x64.var(0, unbiased=False) + EPS).rsqrt()]).float().contiguous()
    a64 = torch.relu((x64 - mi[:K].double()) * mi[K:].double() * gamma.double() + beta.double())
    a32 = torch.relu((x - mi[:K]) * mi[K:] * gamma + beta)
    wf = ext.linear_split_pack(w, N, K)
    y = torch.full((T, N), float("nan"), device="cuda")
    ext.gemm_split_bn(x, wf, y, T, K, N, in_bn=(mi, gamma, beta))
    within_rule("gemm prologue %dx256x256 y" % T, y, a64 @ w.double().t(), a32 @ w.t())
    dw = torch.empty(N, K, device="cuda")
    ext.linear_wgrad_bn(x, gz, dw, T, K, N, mi, gamma, beta)
    within_rule("wgrad prologue %dx256x256 dw" % T, dw, gz.double().t() @ a64, gz.t() @ a32)
    g = _chan(kinds, "g", "cuda")
    assert not dw[:, g].any()                      # a dead input channel contributes exactly nothing


# ------------------------------------------------------------------------------------------------ narrow SA chain
def _chain_f32(xyz, new_xyz, feats, idx, mlp):
    """The chain of tests/test_sa_small_train.py::_reference_fp64 with torch's own f32 operators."""
    B, M, ns = idx.shape
    ii = idx.long()
    gx = torch.stack([xyz[b][ii[b]] for b in range(B)]) - new_xyz.unsqueeze(2)
    gf = torch.stack([feats[b][ii[b]] for b in range(B)])
    x = torch.cat([gx, gf], dim=-1)
    layers, run = list(mlp), []
    for k in range(3):
        conv, bn = layers[3 * k], layers[3 * k + 1]
        z = x @ conv.weight.flatten(1).t()
        rm, rv = torch.zeros_like(bn.running_mean), torch.ones_like(bn.running_var)
        x = torch.relu(F.batch_norm(z.view(-1, z.shape[-1]), rm, rv, bn.weight, bn.bias, True, bn.momentum, bn.eps)).view(z.shape)
        run.append((rm, rv))
    return x.max(dim=2)[0], run


@gpu
@pytest.mark.parametrize("offset,translate", [(0.0, False), (30.0, False), (1000.0, False), (30.0, True)])
def test_sa_small_chain_offset_feature_and_translated_scene(offset, translate):
    """pu.sa_small_chain_train on case ((4, 32, 16, 64), 32, 1, 1000, 96) of tests/test_sa_small_train.py with the raw
    feature channel = offset + N(0, 1) (a 0-255 intensity, a timestamp, an absolute height), and with the scene moved by
    (+70, -40, +3) m: only coordinate differences enter the chain, so that must change nothing beyond rounding."""
    from pdanet_amd import pointnet2_utils as pu
    from test_sa_small_train import _mlp, _reference_fp64, _scene
    dims, ns, B, N, M = (4, 32, 16, 64), 32, 1, 1000, 96
    xyz, _ = _scene(B, N, seed=11 + ns)
    if translate:
        xyz = (xyz + torch.tensor([70.0, -40.0, 3.0], device="cuda")).contiguous()
    feats = (offset + torch.randn(B, N, 1, generator=torch.Generator().manual_seed(12))).cuda()
    new_xyz = xyz[:, :M].contiguous()
    idx = pu.ball_query(1.6, ns, xyz, new_xyz)
    mlp = _mlp(dims, seed=dims[1] + ns)
    assert pu.SaSmallChainTrain.supported(xyz, new_xyz, feats, idx, mlp)
    params = list(mlp.parameters())
    out = pu.sa_small_chain_train(xyz, new_xyz, feats, idx, mlp)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).cuda()
    gk = torch.autograd.grad(out, params, gout)
    ref, stats = _reference_fp64(xyz, new_xyz, feats, idx, mlp)
    g64 = torch.autograd.grad(ref, params, gout.double())
    lib, run = _chain_f32(xyz, new_xyz, feats, idx, mlp)
    g32 = torch.autograd.grad(lib, params, gout)
    tag = "sa_small_chain offset=%g%s " % (offset, " translated" if translate else "")
    within_rule(tag + "out", out, ref, lib)
    for k, bn in enumerate(list(mlp)[1::3]):
        mean, var_u = stats[k]
        within_rule(tag + "running_mean[%d]" % k, bn.running_mean, MOM32 * mean.detach(), run[k][0])
        within_rule(tag + "running_var[%d]" % k, bn.running_var, (1.0 - MOM32) + MOM32 * var_u.detach(), run[k][1])
    for (n, _), a, b, t in zip(mlp.named_parameters(), gk, g64, g32):
        within_rule(tag + "d " + n, a, b, t)


# ------------------------------------------------------------------------------------------------ DensityNet
@gpu
@pytest.mark.parametrize("profile", ["50+rand", "1e-6*rand"])
def test_densitynet_offset_and_tiny_inputs(profile):
    from pdanet_amd import pointnet2_modules as pm, pointnet2_utils as pu
    shape = (2, 300, 16, 1)
    torch.manual_seed(316)
    dn = pm.DensityNet().cuda().train()
    with torch.no_grad():
        for b in dn.mlp_bns:
            b.weight.uniform_(0.5, 1.5); b.bias.normal_(0, 0.3)
    twins = {}
    for dt in (torch.float64, torch.float32):
        m = pm.DensityNet().cuda().to(dt).train()
        m.load_state_dict({k: (v.to(dt) if v.is_floating_point() else v) for k, v in dn.state_dict().items()})
        twins[dt] = m
    r = torch.rand(shape, device="cuda")
    x = 50.0 + r if profile == "50+rand" else 1e-6 * r
    assert pu.DensityNetFused.supported(x, dn)
    y = pu.densitynet(dn, x)
    y64 = twins[torch.float64](x.double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    y32 = twins[torch.float32](x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    go = torch.randn_like(y) * _margin(y64).float()          # the last ReLU: y64 == 0 or tiny -> no gradient
    gk = torch.autograd.grad(y, list(dn.parameters()), go)
    g64 = torch.autograd.grad(y64, list(twins[torch.float64].parameters()), go.double())
    g32 = torch.autograd.grad(y32, list(twins[torch.float32].parameters()), go)
    tag = "densitynet %s " % profile
    within_rule(tag + "y", y, y64, y32)
    for i in range(3):
        for q in ("running_mean", "running_var"):
            within_rule(tag + "%s[%d]" % (q, i), getattr(dn.mlp_bns[i], q), getattr(twins[torch.float64].mlp_bns[i], q),
                        getattr(twins[torch.float32].mlp_bns[i], q))
    for (n, _), a, b, t in zip(dn.named_parameters(), gk, g64, g32):
        within_rule(tag + "d " + n, a, b, t)


# ------------------------------------------------------------------------------------------------ LayerNorm
@gpu
@pytest.mark.parametrize("d", [256, 512, 1024])
@pytest.mark.parametrize("residual", [False, True])
def test_layer_norm_hostile_rows(d, residual):
    from pdanet_amd import pointnet2_utils as pu, pointnet2_batch_cuda as ext
    rows = 77
    x, res, gamma, beta, kinds = ln_profiles(rows, d, seed=d + residual, residual=residual)
    x, gamma, beta = x.cuda(), gamma.cuda(), beta.cuda()
    res = None if res is None else res.cuda()
    gy = torch.randn(rows, d, device="cuda", generator=torch.Generator("cuda").manual_seed(8))

    def twin(dt):
        leaves = [_leaf(t, dt) for t in ((x, gamma, beta) if res is None else (x, gamma, beta, res))]
        s = leaves[0] if res is None else leaves[0] + leaves[3]
        yy = F.layer_norm(s, (d,), leaves[1], leaves[2], EPS)
        return yy, torch.autograd.grad(yy, leaves, gy.to(dt))
    y64, g64 = twin(torch.float64)
    y32, g32 = twin(torch.float32)
    ln = torch.nn.LayerNorm(d, eps=EPS).cuda()
    with torch.no_grad():
        ln.weight.copy_(gamma); ln.bias.copy_(beta)
    xk = x.clone().requires_grad_(True)
    rk = None if res is None else res.clone().requires_grad_(True)
    assert pu.LayerNormResidual.supported(xk, d)
    y = pu.layer_norm(xk, ln, rk)
    gk = torch.autograd.grad(y, [xk, ln.weight, ln.bias] + ([] if rk is None else [rk]), gy)
    tag = "layer_norm 77x%d%s " % (d, " +residual" if residual else "")
    within_rule(tag + "y", y, y64, y32)
    for n, a, b, t in zip(("dx", "dgamma", "dbeta", "dresidual"), gk, g64, g32):
        within_rule(tag + n, a, b, t)
    const = torch.tensor([r for r, k in enumerate(kinds) if k == "constant"], device="cuda")
    assert torch.equal(y.detach()[const], beta.expand(const.numel(), d)), tag + ": constant row, y != beta"
    # the bf16-output entry: same statistics, bf16 copies of y and grad_x
    s_out = torch.empty(rows, d, device="cuda") if res is not None else None
    yf, st = torch.empty(rows, d, device="cuda"), torch.empty(rows, 2, device="cuda")
    yb = torch.empty(rows, d, device="cuda", dtype=torch.bfloat16)
    ext.layer_norm_fwd(x, res, gamma, beta, s_out, yf, st, rows, d, EPS, y_bf16=yb)
    within_rule(tag + "y(bf16)", yb, y64, y32.bfloat16())
    assert torch.equal(yb[const], beta.bfloat16().expand(const.numel(), d))
    scratch = torch.empty(ext.layer_norm_scratch_bytes(d), dtype=torch.uint8, device="cuda")
    gx, gg, gb = torch.empty(rows, d, device="cuda"), torch.empty(d, device="cuda"), torch.empty(d, device="cuda")
    gxb = torch.empty(rows, d, device="cuda", dtype=torch.bfloat16)
    ext.layer_norm_bwd(x if res is None else s_out, gy, gamma, st, gx, gg, gb, scratch, rows, d, grad_x_bf16=gxb)
    within_rule(tag + "dx(bf16)", gxb, g64[0], g32[0].bfloat16())
    within_rule(tag + "dgamma (bf16 entry)", gg, g64[1], g32[1])


# ------------------------------------------------------------------------------------------------ attention
def _dense_kernel(qkv, heads, go):
    from pdanet_amd import pointnet2_batch_cuda as ext
    G, S, D3 = qkv.shape
    hd = D3 // (3 * heads)
    out = torch.empty(G, S, heads * hd, device="cuda")
    lse = torch.empty(G, heads, S, device="cuda")
    ext.group_attention_fwd(qkv, out, lse, G, S, heads, hd)
    dq = torch.empty_like(qkv)
    ext.group_attention_bwd(qkv, go, lse, dq, G, S, heads, hd)
    torch.cuda.synchronize()
    return out, lse, dq


@gpu
@pytest.mark.parametrize("S,hd,heads,G", ATT_SHAPES)
def test_group_attention_dense(S, hd, heads, G):
    """pu.group_attention (and the lse of ext.group_attention_fwd) on the profile groups; isolation between the groups
    that share a 32-row tile; permutation of a group's tokens."""
    from pdanet_amd import pointnet2_utils as pu
    qkv, kinds = att_profiles(S, hd, heads, G, seed=S + hd)
    qkv = qkv.cuda()
    go = torch.randn(G, S, heads * hd, device="cuda", generator=torch.Generator("cuda").manual_seed(9))
    tag = "attention dense S=%d hd=%d " % (S, hd)

    def check(q_in, go_in, label):
        l64, o64, lse64 = attention_twin(q_in, heads, torch.float64)
        l32, o32, lse32 = attention_twin(q_in, heads, torch.float32)
        (d64,) = torch.autograd.grad(o64, l64, go_in.double())
        (d32,) = torch.autograd.grad(o32, l32, go_in)
        qk = q_in.clone().requires_grad_(True)
        assert pu.GroupAttention.supported(qk, heads)
        out = pu.group_attention(qk, heads)
        (dq,) = torch.autograd.grad(out, qk, go_in)
        out2, lse, dq2 = _dense_kernel(q_in, heads, go_in)
        assert torch.equal(out2, out.detach()) and torch.equal(dq2, dq)
        within_rule(tag + label + "out", out, o64, o32)
        within_rule(tag + label + "lse", lse, lse64, lse32)
        within_rule(tag + label + "dqkv", dq, d64, d32)
        return out.detach(), lse, dq
    out, lse, dq = check(qkv, go, "")
    # isolation: one control group scaled by 1e3 (finite) leaves every other group's rows bit-identical
    g0 = 6 if G > 6 else 0
    assert kinds[g0] == "control"
    q2 = qkv.clone()
    q2[g0] *= 1e3
    out2, lse2, dq2 = _dense_kernel(q2, heads, go)
    others = torch.arange(G, device="cuda") != g0
    assert torch.equal(out2[others], out[others]) and torch.equal(lse2[others], lse[others]) and torch.equal(dq2[others], dq[others])
    # key permutation: permuting the S tokens of every group permutes its outputs (each side of the rule sees the same input)
    perm = torch.randperm(S, generator=torch.Generator().manual_seed(S)).cuda()
    check(qkv[:, perm].contiguous(), go[:, perm].contiguous(), "permuted ")


@gpu
@pytest.mark.parametrize("S,hd,heads,G", ATT_SHAPES)
def test_group_attention_ragged(S, hd, heads, G):
    """ext.group_attention_ragged_fwd / bwd on compact rows (plans from tests/test_ragged_tokens.py::padded_idx) against
    fp64 dense attention on the padded groups: slot s >= cnt repeats token 0, so a group with cnt == 1 puts log S on its
    single key."""
    from pdanet_amd import pointnet2_utils as pu, pointnet2_batch_cuda as ext
    from test_ragged_tokens import padded_idx
    D = heads * hd
    rng = np.random.default_rng(S + hd + G)
    idx, cnt = padded_idx(G, S, 4000, rng, empty_rows=1)
    cnt[-1] = S; idx[-1] = np.arange(S, dtype=np.int32) * 3 + 1            # a full group whatever the draw
    assert (cnt == 1).any() and (cnt == S).any()
    (plan,) = pu.ragged_plans([torch.from_numpy(idx).cuda().view(1, G, S)])
    U = plan.tokens
    assert np.array_equal(plan.cnt.cpu().numpy(), cnt)
    dense, kinds = att_profiles(S, hd, heads, G, seed=S + hd + 1)
    qkv_c = dense.cuda().view(G * S, 3 * D)[plan.rowmap.long()].contiguous()                 # (U, 3D)
    go_c = torch.randn(U, D, device="cuda", generator=torch.Generator("cuda").manual_seed(10))
    off = plan.off.long()[:-1]
    slot = torch.arange(S, device="cuda").view(1, S)
    valid = slot < plan.cnt.long().view(G, 1)
    src = off.view(G, 1) + torch.where(valid, slot, torch.zeros_like(slot))

    def twin(dt, q_c):
        leaf = _leaf(q_c, dt)
        G_, S_ = src.shape
        qd = leaf[src]                                                                    # (G, S, 3D): copies share the leaf row
        q, k, v = qd.view(G_, S_, 3, heads, hd).permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
        if dt == torch.float64:
            o = torch.softmax(s, dim=-1) @ v
        else:
            from torch.nn.attention import SDPBackend, sdpa_kernel
            with sdpa_kernel(SDPBackend.MATH):
                o = F.scaled_dot_product_attention(q, k, v)
        o = o.transpose(1, 2).reshape(G_, S_, D)[valid]                                   # (U, D)
        (dq,) = torch.autograd.grad(o, leaf, go_c.to(dt))
        return o.detach(), torch.logsumexp(s.detach(), dim=-1), dq

    def kernel(q_c):
        out = torch.empty(U, D, device="cuda"); lse = torch.zeros(G, heads, S, device="cuda")
        ext.group_attention_ragged_fwd(q_c, plan.cnt, plan.off, out, lse, U, G, S, heads, hd)
        dq = torch.empty_like(q_c)
        ext.group_attention_ragged_bwd(q_c, go_c, lse, plan.cnt, plan.off, dq, U, G, S, heads, hd)
        torch.cuda.synchronize()
        return out, lse, dq
    o64, lse64, d64 = twin(torch.float64, qkv_c)
    o32, lse32, d32 = twin(torch.float32, qkv_c)
    out, lse, dq = kernel(qkv_c)
    tag = "attention ragged S=%d hd=%d " % (S, hd)
    vm = valid.view(G, 1, S).expand(G, heads, S)
    within_rule(tag + "out", out, o64, o32)
    within_rule(tag + "lse", lse[vm], lse64[vm], lse32[vm])
    within_rule(tag + "dqkv", dq, d64, d32)
    # isolation on the compact rows
    g0 = 6 if G > 6 else 0
    assert kinds[g0] == "control"
    mine = torch.zeros(U, dtype=torch.bool, device="cuda")
    mine[int(plan.off[g0]):int(plan.off[g0 + 1])] = True
    q2 = qkv_c.clone()
    q2[mine] *= 1e3
    out2, lse2, dq2 = kernel(q2)
    og = torch.arange(G, device="cuda") != g0
    assert torch.equal(out2[~mine], out[~mine]) and torch.equal(dq2[~mine], dq[~mine])
    assert torch.equal(lse2[og][vm[og]], lse[og][vm[og]])
