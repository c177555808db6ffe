"""-m gpu: every kernel of the unique-token ("ragged") PDA path against a dense statement of the same operation in plain
torch ops on the same device -- csrc/ragged.hip (plan, token assembly forward and backward, add + max-pool, its scatter) and
RaggedTransformerBlock as one node.  No reference here is another kernel of this repository.

The dense twin every test builds from a plan: slot s of group g reads compact row src[g, s] = off[g] + (s if s < cnt[g]
else 0), valid[g, s] = s < cnt[g].  Copies share a row, so autograd through x_c[src] sums their gradients.

  1. plan            cnt / off / rowmap / roww exactly equal to numpy, nothing written at or beyond U; the padding
                     convention of the neighbour search that ragged_count_kernel relies on, on a real neighbour list.
  2. assembly fwd    bit for bit (copies and one f32 multiply), B > 1, all five channel counts, both rppe layouts.
  3. assembly bwd    both forms; on integer data bit for bit against fp64 autograd (integer sums are exact in any order, so
                     a dropped or doubled float-atomic contribution cannot hide); on normal data within the f32 summation
                     bound (terms + 8) * 2^-24 * sum|terms| per element, the form tests/test_sparse_conv.py uses.
  4. pool / scatter  bit for bit, first maximum on ties, -inf channels, every element of the U rows written, none beyond.
  5. block node      out, dx and the twelve parameter gradients under tests/test_hostile_numerics.py::within_rule
                     (e_k <= 3 * e_t + 4 * 2^-24 * scale against fp64, e_t = the same statement in torch's own f32 ops).

Largest e_k / e_t observed on MI355X in group 5, per quantity over the four shapes (within_rule prints every one; it
accepts 3 plus the floor term):
  out 1.43   dx 0.76   norm1.weight 1.43   norm1.bias 2.12   in_proj_weight 0.42   in_proj_bias 2.74   out_proj.weight 1.04
  out_proj.bias 1.84   norm2.weight 1.42   norm2.bias 1.85   linear1.weight 1.14   linear1.bias 1.85   linear2.weight 1.24
  linear2.bias 1.09
Every figure above 1.5 except out_proj.bias (1.84 at (77, 8, 256, 128)) is a column sum over the U = 8182 rows of
(900, 16, 256, 128): the bias gradients of csrc/wgrad.hip and the LayerNorm bias gradients of csrc/layer_norm.hip.  The nearest
to its bar is in_proj_bias there, e_k = 4.3e-5 against 6.2e-5.  The three shapes below 4096 tokens stay at or below 1.43 otherwise.
Largest error / bound on normal data in group 3: grad_glob 0.16, grad_dscale 0.03, grad_feats 0.23."""
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
from test_hostile_numerics import U32, _margin, within_rule  # noqa: E402
from test_ragged_tokens import padded_idx  # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ numpy / torch helpers
def plan_numpy(idx):
    """idx (G, S) int32 -> cnt, off, rowmap, roww as the plan defines them, from the distinct values of every row."""
    G, S = idx.shape
    cnt = np.array([len(np.unique(r)) for r in idx], np.int32)
    off = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)]).astype(np.int32)
    rowmap = np.concatenate([g * S + np.arange(c) for g, c in enumerate(cnt)]).astype(np.int32)
    roww = np.ones(int(off[-1]), np.float32)
    roww[off[:-1]] = (S - cnt + 1).astype(np.float32)
    return cnt, off, rowmap, roww


def padding_convention(idx):
    """idx (G, S): per row the length c of its strictly ascending head, and whether the rest repeats the first entry."""
    G, S = idx.shape
    same = idx == idx[:, :1]
    rep = np.concatenate([same[:, 1:], np.ones((G, 1), bool)], axis=1)            # a stop behind the last slot
    c = (1 + np.argmax(rep, axis=1)).astype(np.int32)                              # the first repeat of entry 0 ends the head
    slot = np.arange(S)[None, :]
    head = slot < c[:, None]
    asc = (np.diff(idx.astype(np.int64), axis=1) > 0) | ~head[:, 1:]
    tail = same | head
    return c, asc.all(1) & tail.all(1)


def dense_twin(cnt, off, S):
    """src (G, S) long, valid (G, S) bool from a plan's cnt (G) and off (G + 1)."""
    G = cnt.shape[0]
    slot = torch.arange(S, device=cnt.device).view(1, S)
    valid = slot < cnt.long().view(G, 1)
    src = off.long()[:-1].view(G, 1) + torch.where(valid, slot, torch.zeros_like(slot))
    return src, valid


def forced_idx(G, S, n, rng, p_single=0.3, p_full=0.1):
    """padded_idx with a cnt = 1 group (group 0: the ball without a hit) and a cnt = S group (the last one) whatever the
    draw; a single group is the full one."""
    idx, cnt = padded_idx(G, S, n, rng, p_single, p_full, empty_rows=1 if G > 1 else 0)
    cnt[-1] = S
    idx[-1] = np.arange(S, dtype=np.int32) * 3 + 1
    assert (cnt == S).any() and (G == 1 or (cnt == 1).any())
    return idx, cnt


def _plan(idx_np, shape):
    from pdanet_amd import pointnet2_utils as pu
    idx_t = torch.from_numpy(idx_np).cuda().view(shape)
    (plan,) = pu.ragged_plans([idx_t])
    cnt, off, rowmap, _ = plan_numpy(idx_np.reshape(-1, shape[-1]))                # the references stand on numpy's plan
    assert np.array_equal(plan.cnt.cpu().numpy(), cnt) and np.array_equal(plan.off.cpu().numpy(), off)
    assert np.array_equal(plan.rowmap.cpu().numpy(), rowmap)
    return idx_t, plan


# ------------------------------------------------------------------------------------------------ 1. plan
PLAN_SHAPES = [(1, 1, 8), (3, 341, 16), (1, 1024, 32), (5, 205, 8), (1, 2049, 1), (2, 33, 255)]


@pytest.mark.parametrize("B,M,S", PLAN_SHAPES)
def test_plan_equals_numpy_and_writes_nothing_beyond_U(B, M, S):
    """(3, 341, 16): G = 1023, one group per thread of the one-workgroup scan with the last thread idle; (5, 205, 8): G = 1025,
    two groups per thread; (1, 2049, 1): every cnt = 1; (2, 33, 255): the largest nsample the entry accepts."""
    from pdanet_amd import pointnet2_utils as pu, pointnet2_batch_cuda as ext
    G = B * M
    rng = np.random.default_rng(1000 * B + M + S)
    idx = padded_idx(G, S, 5000, rng)[0].reshape(B, M, S)
    cnt, off, rowmap, roww = plan_numpy(idx.reshape(G, S))
    U = int(off[-1])
    idx_t = torch.from_numpy(idx).cuda()
    k_cnt = torch.full((G,), -7, dtype=torch.int32, device="cuda")
    k_off = torch.full((G + 1,), -7, dtype=torch.int32, device="cuda")
    k_map = torch.full((G * S,), -7, dtype=torch.int32, device="cuda")
    k_w = torch.full((G * S,), -7.0, dtype=torch.float32, device="cuda")
    ext.ragged_plan(idx_t, k_cnt, k_off, k_map, G, S, k_w)
    assert np.array_equal(k_cnt.cpu().numpy(), cnt)
    assert np.array_equal(k_off.cpu().numpy(), off)
    assert np.array_equal(k_map[:U].cpu().numpy(), rowmap)
    assert np.array_equal(k_w[:U].cpu().numpy(), roww)
    assert float(k_w[:U].double().sum()) == G * S
    assert bool((k_map[U:] == -7).all()) and bool((k_w[U:] == -7.0).all())
    # the plan object the layers use, from the (B, M, S) tensor
    (plan,) = pu.ragged_plans([idx_t])
    assert (plan.tokens, plan.groups, plan.nsample) == (U, G, S)
    assert torch.equal(plan.cnt, k_cnt) and torch.equal(plan.off, k_off)
    assert torch.equal(plan.rowmap, k_map[:U]) and torch.equal(plan.roww, k_w[:U])
    assert plan.rowmap.numel() == U and plan.roww.numel() == U


def test_plan_count_rests_on_the_neighbour_searchs_padding():
    """ragged_count_kernel counts the entries that differ from the first one.  That is the number of distinct neighbours only
    while the search leaves c strictly ascending indices followed by repeats of the first: pinned here on the scene of
    tests/test_ragged_tokens.py::test_pda_layer_ragged_equals_dense, both scales."""
    from pdanet_amd import pointnet2_utils as pu, synth
    xyz = torch.from_numpy(synth.batch_xyz(2, 4096, config_id=2)).cuda()
    new_xyz = xyz[:, :1024].contiguous()
    idxs = pu.ball_query_multi([0.8, 1.6], [16, 32], xyz, new_xyz)
    plans = pu.ragged_plans(idxs)
    for idx_t, plan, ns in zip(idxs, plans, (16, 32)):
        idx = idx_t.cpu().numpy().reshape(-1, ns)
        assert idx.shape[0] == 2048 and idx.min() >= 0 and idx.max() < 4096
        c, ok = padding_convention(idx)
        assert ok.all(), "rows that are not an ascending head followed by repeats of the first: %s" % np.nonzero(~ok)[0][:8]
        distinct = np.array([len(np.unique(r)) for r in idx], np.int32)
        assert np.array_equal(c, distinct)
        assert np.array_equal(plan.cnt.cpu().numpy(), distinct)
        assert plan.tokens == int(distinct.sum())
        assert (c == 1).any() and (c == ns).any()


# ------------------------------------------------------------------------------------------------ 2. / 3. token assembly
ASM_SHAPES = [(1, 40, 5, 16, 16, False), (2, 300, 129, 8, 64, True), (3, 257, 67, 32, 128, False), (2, 64, 33, 1, 256, True),
              (2, 500, 100, 3, 32, False)]


def assembly_statement(rppe, dscale, feats, glob, idx, rowmap, compact):
    """The assembled compact rows (U, 4C) in plain torch ops, in the dtype of the operands: [rppe | f * dscale | f | glob]
    of every dense slot, then the rows the plan keeps.  rppe: (B,M,S,C) dense, or (U,C) compact (scattered to its slots)."""
    B, M, S = idx.shape
    C = feats.shape[-1]
    ii = idx.long()
    g = torch.stack([feats[b][ii[b]] for b in range(B)])                          # (B, M, S, C)
    if compact:
        rppe_d = torch.zeros(B * M * S, C, dtype=rppe.dtype, device=rppe.device).index_copy(0, rowmap.long(), rppe).view(B, M, S, C)
    else:
        rppe_d = rppe
    x = torch.cat([rppe_d, g * dscale, g, glob.unsqueeze(2).expand(B, M, S, C)], -1)
    return x.view(B * M * S, 4 * C)[rowmap.long()]


def _assembly_case(B, N, M, ns, C, compact, integers, seed):
    rng = np.random.default_rng(seed)
    idx = padded_idx(B * M, ns, N, rng)[0].reshape(B, M, ns)
    idx_t, plan = _plan(idx, (B, M, ns))
    U = plan.tokens
    gen = torch.Generator().manual_seed(seed)
    if integers:
        def draw(*shape):
            return torch.randint(-8, 9, shape, generator=gen).float().cuda()
        dscale = torch.randint(0, 4, (B, M, ns, 1), generator=gen).float().cuda()
    else:
        def draw(*shape):
            return torch.randn(*shape, generator=gen).cuda()
        dscale = (torch.rand(B, M, ns, 1, generator=gen) * 0.998 + 0.001).cuda()
    rppe = draw(U, C) if compact else draw(B, M, ns, C)
    feats, glob, go = draw(B, N, C), draw(B, M, C), draw(U, 4 * C)
    return idx_t, plan, rppe, dscale, feats, glob, go


@pytest.mark.parametrize("B,N,M,ns,C,compact", ASM_SHAPES)
def test_assembly_forward_bit_for_bit(B, N, M, ns, C, compact):
    from pdanet_amd import pointnet2_utils as pu, pointnet2_batch_cuda as ext
    idx_t, plan, rppe, dscale, feats, glob, _ = _assembly_case(B, N, M, ns, C, compact, False, seed=B + N + M + ns + C)
    U = plan.tokens
    want = assembly_statement(rppe, dscale, feats, glob, idx_t, plan.rowmap, compact)
    buf = torch.full((U + 3, 4 * C), float("nan"), device="cuda")
    out = buf[:U]
    ext.assemble_tokens_ragged(rppe, dscale, feats, idx_t, glob, plan.rowmap, plan.off, out, U, B, N, M, ns, C, rppe_compact=compact)
    assert not torch.isnan(out).any()
    assert torch.isnan(buf[U:]).all()
    assert torch.equal(out, want)
    assert torch.equal(pu.AssembleTokensRagged.apply(rppe, dscale, feats, idx_t, glob, plan), want)


def _assembly_grads_fp64(idx_t, plan, rppe, dscale, feats, glob, go, compact):
    leaves = [t.detach().double().requires_grad_(True) for t in (rppe, dscale, feats, glob)]
    x = assembly_statement(leaves[0], leaves[1], leaves[2], leaves[3], idx_t, plan.rowmap, compact)
    return torch.autograd.grad(x, leaves, go.double())


def _assembly_grads_kernel(idx_t, plan, rppe, dscale, feats, go, compact, with_rowmap):
    """The entry point itself, into buffers it has to fill: NaN wherever it writes, zeros where it accumulates."""
    from pdanet_amd import pointnet2_batch_cuda as ext
    B, M, ns = idx_t.shape
    N, C = feats.shape[1], feats.shape[2]
    U = plan.tokens
    nan = float("nan")
    g_rppe = torch.full((U, C) if compact else (B, M, ns, C), nan, device="cuda")
    g_ds = torch.full((B, M, ns, 1), nan, device="cuda")
    g_feats = torch.zeros(B, N, C, device="cuda")
    g_glob = torch.full((B, M, C), nan, device="cuda")
    ext.assemble_tokens_ragged_grad(go, dscale, feats, idx_t, plan.cnt, plan.off, g_rppe, g_ds, g_feats, g_glob, U, B, N, M, ns, C,
                                    rppe_compact=compact, rowmap=plan.rowmap if with_rowmap else None)
    return g_rppe, g_ds, g_feats, g_glob


@pytest.mark.parametrize("with_rowmap", [True, False])
@pytest.mark.parametrize("B,N,M,ns,C,compact", ASM_SHAPES)
def test_assembly_backward_integers_bit_for_bit(B, N, M, ns, C, compact, with_rowmap):
    """Integers in [-8, 8], dscale in {0..3}: every product and partial sum is a small integer, so f32 in any order equals
    fp64.  |grad_dscale| <= 64 C, |grad_feats| <= 32 P, |grad_glob| <= 8 ns: far below 2^24."""
    from pdanet_amd import pointnet2_utils as pu
    idx_t, plan, rppe, dscale, feats, glob, go = _assembly_case(B, N, M, ns, C, compact, True, seed=B + N + M + ns + C + 1)
    ref = _assembly_grads_fp64(idx_t, plan, rppe, dscale, feats, glob, go, compact)
    got = _assembly_grads_kernel(idx_t, plan, rppe, dscale, feats, go, compact, with_rowmap)
    for name, a, b in zip(("grad_rppe", "grad_dscale", "grad_feats", "grad_glob"), got, ref):
        assert torch.equal(a, b.float()), name
    _, valid = dense_twin(plan.cnt, plan.off, ns)
    repeat = ~valid.view(B, M, ns)
    assert not got[1].view(B, M, ns)[repeat].any()
    if not compact:
        assert not got[0][repeat].any()
    # the autograd node the layers call, in the form the switch selects
    old = pu.ASSEMBLE_BWD_TOKEN_PARALLEL
    try:
        pu.ASSEMBLE_BWD_TOKEN_PARALLEL = with_rowmap
        leaves = [t.clone().requires_grad_(True) for t in (rppe, dscale, feats, glob)]
        x = pu.AssembleTokensRagged.apply(leaves[0], leaves[1], leaves[2], idx_t, leaves[3], plan)
        node = torch.autograd.grad(x, leaves, go)
    finally:
        pu.ASSEMBLE_BWD_TOKEN_PARALLEL = old
    for name, a, b in zip(("rppe", "dscale", "feats", "glob"), node, ref):
        assert torch.equal(a, b.float()), "AssembleTokensRagged.backward " + name


def assembly_bounds(idx_t, plan, dscale, feats, go):
    """fp64 per-element bounds (terms + 8) * 2^-24 * sum|terms| of the three summed gradients, and P (B, N): the number of
    compact tokens that reference a point."""
    B, M, ns = idx_t.shape
    N, C = feats.shape[1], feats.shape[2]
    rm = plan.rowmap.long()
    g = go.double().abs()
    g_fd, g_f, g_g = g[:, C:2 * C], g[:, 2 * C:3 * C], g[:, 3 * C:]
    group = rm // ns
    point = (group // M) * N + idx_t.reshape(-1).long()[rm]                        # row of feats.view(B * N, C)
    d = dscale.double().reshape(-1)[rm].abs().unsqueeze(1)
    f = feats.double().reshape(B * N, C)[point].abs()
    s_glob = torch.zeros(B * M, C, dtype=torch.float64, device=go.device).index_add_(0, group, g_g)
    b_glob = (plan.cnt.double().view(B * M, 1) + 8) * U32 * s_glob
    b_ds = torch.zeros(B * M * ns, dtype=torch.float64, device=go.device)
    b_ds[rm] = (C + 8) * U32 * (g_fd * f).sum(1)
    P = torch.zeros(B * N, dtype=torch.float64, device=go.device).index_add_(0, point, torch.ones_like(point, dtype=torch.float64))
    s_feats = torch.zeros(B * N, C, dtype=torch.float64, device=go.device).index_add_(0, point, g_fd * d + g_f)
    b_feats = (P.unsqueeze(1) + 8) * U32 * s_feats
    return b_glob.view(B, M, C), b_ds.view(B, M, ns, 1), b_feats.view(B, N, C), P.view(B, N)


@pytest.mark.parametrize("with_rowmap", [True, False])
@pytest.mark.parametrize("B,N,M,ns,C,compact", ASM_SHAPES)
def test_assembly_backward_normal_data_within_summation_bound(B, N, M, ns, C, compact, with_rowmap):
    idx_t, plan, rppe, dscale, feats, glob, go = _assembly_case(B, N, M, ns, C, compact, False, seed=B + N + M + ns + C + 2)
    ref = _assembly_grads_fp64(idx_t, plan, rppe, dscale, feats, glob, go, compact)
    got = _assembly_grads_kernel(idx_t, plan, rppe, dscale, feats, go, compact, with_rowmap)
    b_glob, b_ds, b_feats, P = assembly_bounds(idx_t, plan, dscale, feats, go)
    assert torch.equal(got[0], ref[0].float()), "grad_rppe is a copy"
    for name, a, r, bound in (("grad_dscale", got[1], ref[1], b_ds), ("grad_feats", got[2], ref[2], b_feats),
                              ("grad_glob", got[3], ref[3], b_glob)):
        assert torch.isfinite(a).all(), name
        err = (a.double() - r).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
        print("RAGGED assembly bwd %s rowmap=%s %-11s max err / bound = %.3f" % ((B, N, M, ns, C), with_rowmap, name, ratio))
        assert bool((err <= bound).all()), "%s: err / bound = %.3f" % (name, ratio)
    assert not got[2][P == 0].any(), "a point no token references received a gradient"
    _, valid = dense_twin(plan.cnt, plan.off, ns)
    assert not got[1].view(B, M, ns)[~valid.view(B, M, ns)].any()


# ------------------------------------------------------------------------------------------------ 4. pool and scatter
POOL_SHAPES = [(1, 8, 4), (65, 16, 64), (333, 32, 256), (77, 8, 1024)]


def pool_statement(v, src, valid):
    """v (U, D) compact -> max over the valid slots of every group (G, D) and the first slot that attains it."""
    d = v[src]                                                                        # (G, S, D)
    d = torch.where(valid.unsqueeze(-1), d, torch.full((), -math.inf, dtype=v.dtype, device=v.device))
    m = d.max(dim=1)[0]
    first = (d == m.unsqueeze(1)).int().argmax(1)
    return m, first


@pytest.mark.parametrize("G,S,D", POOL_SHAPES)
def test_pool_and_scatter_bit_for_bit(G, S, D):
    from pdanet_amd import pointnet2_batch_cuda as ext
    rng = np.random.default_rng(G + S + D)
    idx, _ = forced_idx(G, S, 4000, rng)
    _, plan = _plan(idx, (1, G, S))
    U = plan.tokens
    src, valid = dense_twin(plan.cnt, plan.off, S)
    gen = torch.Generator().manual_seed(G + D)
    a, b = torch.randn(U, D, generator=gen).cuda(), torch.randn(U, D, generator=gen).cuda()
    last = int(plan.off[G - 1])                                                        # the full group: S >= 8 tokens
    a[last + 3] = a[last + 5] = 64.0; b[last + 3] = b[last + 5] = 0.0                   # identical tokens above all others: a tie
    a[last:last + S, 1] = -math.inf                                                    # a channel at -inf on every token of a group
    if G > 1:
        b[0, 2] = -math.inf                                                            # ... and on the one token of a single group
    out = torch.full((G, D), float("nan"), device="cuda")
    arg = torch.full((G, D), 255, dtype=torch.uint8, device="cuda")
    ext.add_max_pool_ragged(a, b, plan.cnt, plan.off, out, arg, U, G, D)
    want, first = pool_statement(a + b, src, valid)
    assert torch.equal(out, want)
    assert torch.equal(arg.long(), first.long())
    tie = torch.ones(D, dtype=torch.bool, device="cuda"); tie[1] = False
    assert bool((arg[G - 1][tie] == 3).all()) and bool((out[G - 1][tie] == 64.0).all())
    assert out[G - 1, 1].item() == -math.inf and arg[G - 1, 1].item() == 0
    if G > 1:
        assert out[0, 2].item() == -math.inf and arg[0, 2].item() == 0
    # scatter
    go = torch.randn(G, D, generator=gen).cuda()
    buf = torch.full((U + 3, D), float("nan"), device="cuda")
    dx = buf[:U]
    ext.max_pool_scatter_ragged(go, arg, plan.rowmap, plan.off, dx, U, G, S, D)
    ref = torch.zeros(G, S, D, device="cuda").scatter_(1, first.unsqueeze(1), go.unsqueeze(1))[valid]
    assert not torch.isnan(dx).any()
    assert torch.isnan(buf[U:]).all()
    assert torch.equal(dx, ref)


# ------------------------------------------------------------------------------------------------ 5. the block as a node
# (G, S, D, ff, heads, p_single, seed).  The seed is one at which no fp64 pre-activation of linear1 lies within RELU_CLEAR of
# zero (asserted in the test), found on the CPU by counting up from 0: the third shape has one at 1.6e-6 under seed 0; the
# last shape has 1.1 million pre-activations, about two of them expected inside the band, and seeds 0-28 each have one
# there except 17, which clears it by a tenth only (2.2e-6); 29 clears it twice over (4.3e-6).
BLOCK_SHAPES = [(203, 16, 256, 128, 4, 0.3, 0), (131, 32, 512, 256, 4, 0.3, 0), (77, 8, 256, 128, 4, 0.3, 1),
                (900, 16, 256, 128, 4, 0.0, 29)]
RELU_CLEAR = 2e-6           # about four times the f32 error of linear1's product
PARAMS = ("norm1.weight", "norm1.bias", "self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight",
          "self_attn.out_proj.bias", "norm2.weight", "norm2.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias")


def block_case(G, S, D, ff, heads, p_single, seed):
    """Everything of a case that is drawn: on the CPU, so the same numbers on every device."""
    from pdanet_amd import pointnet2_modules as pm
    rng = np.random.default_rng(seed * 7919 + G + S + D)
    idx, cnt = forced_idx(G, S, 4000, rng, p_single)
    torch.manual_seed(seed * 7919 + G + D)
    layer = pm.TransformerEncoderLayerPreNorm(d_model=D, nhead=heads, dim_feedforward=ff, dropout=0.0)
    U = int(cnt.sum())
    gen = torch.Generator().manual_seed(seed * 7919 + S)
    return idx, cnt, layer, torch.randn(U, D, generator=gen), torch.randn(G, D, generator=gen)


def block_statement(params, x_c, src, heads, dtype, eps=1e-5):
    """_transformer_batch_first(..., pool=True) in plain torch ops on the dense (G, S, D) tensor x_c[src].  float64: every
    step spelled out; float32: torch's own operators.  Returns the leaf parameters, the leaf x, the values before the pool
    (G, S, D) and the pre-activations of linear1."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    x = x_c.detach().to(dtype).clone().requires_grad_(True)
    G, S = src.shape
    D = x.shape[1]
    hd = D // heads
    xd = x[src]
    s1 = F.layer_norm(xd, (D,), p["norm1.weight"], p["norm1.bias"], eps)
    qkv = F.linear(s1, p["self_attn.in_proj_weight"], p["self_attn.in_proj_bias"])
    q, k, v = qkv.view(G, S, 3, heads, hd).permute(2, 0, 3, 1, 4)
    if dtype == torch.float64:
        a = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(hd), dim=-1) @ v
    else:
        from torch.nn.attention import SDPBackend, sdpa_kernel
        with sdpa_kernel(SDPBackend.MATH):
            a = F.scaled_dot_product_attention(q, k, v)
    a = a.transpose(1, 2).reshape(G, S, D)
    s2 = F.layer_norm(s1 + F.linear(a, p["self_attn.out_proj.weight"], p["self_attn.out_proj.bias"]), (D,),
                      p["norm2.weight"], p["norm2.bias"], eps)
    pre = F.linear(s2, p["linear1.weight"], p["linear1.bias"])
    z = s2 + F.linear(torch.relu(pre), p["linear2.weight"], p["linear2.bias"])
    return p, x, z, pre


def pool_safe(z64, valid):
    """(G, D) bool: the fp64 winner of the pool leads the runner-up among the valid slots by more than the margin."""
    zz = torch.where(valid.unsqueeze(-1), z64.detach(), torch.full((), -math.inf, dtype=z64.dtype, device=z64.device))
    top = zz.topk(2, dim=1)[0]
    return _margin(top[:, 0] - top[:, 1]).bool()


@pytest.mark.parametrize("G,S,D,ff,heads,p_single,seed", BLOCK_SHAPES)
def test_ragged_block_node_against_fp64_statement(G, S, D, ff, heads, p_single, seed):
    from pdanet_amd import pointnet2_utils as pu
    idx, cnt, layer, x_c, go = block_case(G, S, D, ff, heads, p_single, seed)
    layer = layer.cuda()
    x_c, go = x_c.cuda(), go.cuda()
    _, plan = _plan(idx, (1, G, S))
    U = plan.tokens
    assert U == x_c.shape[0]
    if p_single == 0.0:
        assert U >= pu.SPLIT_GEMM_MIN_TOKENS == 4096 and pu.SPLIT_GEMM and pu.LINEAR_WGRAD_KERNEL   # csrc/gemm_split.hip, csrc/wgrad.hip
    else:
        assert U < 4096
    assert pu.RaggedTransformerBlock.supported(D, heads, S, x_c)
    src, valid = dense_twin(plan.cnt, plan.off, S)
    params = dict(layer.named_parameters())
    assert sorted(params) == sorted(PARAMS)
    p64, x64, z64, pre64 = block_statement(params, x_c, src, heads, torch.float64, layer.norm1.eps)
    p32, x32, z32, _ = block_statement(params, x_c, src, heads, torch.float32, layer.norm1.eps)
    # discontinuities: both conditions asserted, nothing hidden
    closest = pre64.detach().abs().min().item()
    assert closest >= RELU_CLEAR, "a linear1 pre-activation %.3e from zero: choose another seed" % closest
    safe = pool_safe(z64, valid)
    share = 1.0 - safe.double().mean().item()
    print("RAGGED block (%d, %d, %d, %d): U = %d, pool entries without gradient %.3f %%, closest pre-activation %.2e"
          % (G, S, D, ff, U, 100 * share, closest))
    assert share <= 0.01
    go = go * safe.float()
    xk = x_c.clone().requires_grad_(True)
    y = pu.ragged_transformer_block(layer, xk, plan)
    gk = torch.autograd.grad(y, [xk] + [params[k] for k in PARAMS], go)
    o64, o32 = z64.max(dim=1)[0], z32.max(dim=1)[0]
    g64 = torch.autograd.grad(o64, [x64] + [p64[k] for k in PARAMS], go.double())
    g32 = torch.autograd.grad(o32, [x32] + [p32[k] for k in PARAMS], go)
    tag = "ragged block (%d,%d,%d,%d) " % (G, S, D, ff)
    within_rule(tag + "out", y, o64, o32)
    for name, a, b, t in zip(("dx",) + tuple("d " + k for k in PARAMS), gk, g64, g32):
        within_rule(tag + name, a, b, t)
