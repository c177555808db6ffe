"""-m gpu: the two fused ends of the wide SA chain (csrc/sa_xyz_grad.hip, PDA_SA_WIDE_FUSED_ENDS):
  * pda_sa_point_gather_stats: sa_point_gather that also emits the BatchNorm statistics of the z1 it stores;
  * pda_bn_relu_bwd_reduce + pda_sa_point_grad_bn: layer 1's backward as one kernel that never writes the gradient at z1;
  * SaWideChainTrain with the switch on against the switch off."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _geometry(b, n, m, ns, seed):
    g = torch.Generator().manual_seed(seed)
    xyz = (torch.rand(b, n, 3, generator=g) * 10).cuda()
    new_xyz = (torch.rand(b, m, 3, generator=g) * 10).cuda()
    return g, xyz, new_xyz


# tokens per workgroup step = 256 / (c1 / 4): 8, 4 and 1; (1, 7, 3, 128): 21 tokens, no multiple of the 8 per step;
# (1, 1, 3, 128): 3 tokens, fewer than one step; (2, 40, 16, 1024): 1280 workgroup steps, more than the grid cap of 1024
@pytest.mark.parametrize("b,m,ns,c1", [(2, 8, 3, 128), (2, 8, 16, 128), (2, 8, 3, 256), (2, 8, 16, 256), (2, 8, 3, 1024), (2, 8, 16, 1024),
                                       (1, 7, 3, 128), (1, 1, 3, 128), (2, 40, 16, 1024)])
def test_gather_stats_z_and_sums(b, m, ns, c1):
    """z1 bit-equal to pda_sa_point_gather's; the summed partials against the fp64 sums of the STORED z1 to 1e-12 relative (the
    bar test_gemm_split_bn_pieces_against_fp64 sets for the GEMM epilogue's sums: both are double sums of floats; the sum itself
    may cancel, so its error is taken relative to the sum of magnitudes); partials bit-equal on a second launch."""
    from pdanet_amd import pointnet2_batch_cuda as ext
    n = 64
    g, xyz, new_xyz = _geometry(b, n, m, ns, 1000 * ns + c1 + m)
    idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32).cuda()
    rows = torch.randn(b * n, c1, generator=g).cuda()
    w = torch.randn(c1, 3 + 5, generator=g).cuda()
    t = b * m * ns
    z_ref = torch.full((t, c1), float("nan"), device="cuda")
    ext.sa_point_gather(rows, xyz, new_xyz, idx, w, z_ref, b, n, m, ns, c1)
    nb = ext.sa_point_gather_stats_blocks(t, c1)
    assert nb == min((t * (c1 // 4) + 255) // 256, 1024)
    parts = []
    for _ in range(2):
        z = torch.full((t, c1), float("nan"), device="cuda")
        part = torch.full((nb * 2 * c1,), float("nan"), dtype=torch.float64, device="cuda")
        ext.sa_point_gather_stats(rows, xyz, new_xyz, idx, w, z, part, b, n, m, ns, c1)
        assert torch.equal(z, z_ref)
        parts.append(part)
    assert torch.equal(parts[0], parts[1])
    p = parts[0].view(nb, 2, c1).sum(0)
    z64 = z_ref.double()
    s1, s2, mag = z64.sum(0), (z64 * z64).sum(0), z64.abs().sum(0)
    e1, e2 = ((p[0] - s1).abs() / mag).max().item(), ((p[1] - s2).abs() / s2).max().item()
    print("sum err / sum|z| %.3e  sum-of-squares rel err %.3e" % (e1, e2))
    assert e1 <= 1e-12 and e2 <= 1e-12


def _bwd_case(ns, c1, m):
    """Inputs of layer 1's backward with the index patterns and channel cases that matter, and the fp64 statement of its outputs."""
    from pdanet_amd import pointnet2_batch_cuda as ext
    b, n = 2, 64
    g, xyz, new_xyz = _geometry(b, n, m, ns, 77 * ns + c1)
    idx = torch.randint(0, 60, (b, m, ns), generator=g, dtype=torch.int32)       # points 60..63: no group references them
    idx[:, :, 0] = 5                                                              # a point shared by every group ...
    idx[0, 0, max(1, ns // 4):] = idx[0, 0, max(1, ns // 4)]                      # padded run: one neighbour repeated to the end
    idx[1, 2, 1:] = idx[1, 2, 0]                                                  # ball-query padding: the first neighbour repeated
    idx[0, 1, :] = 9                                                              # ... but this one: a group that is all one index
    idx = idx.cuda()
    t = b * m * ns
    z = (torch.randn(t, c1, generator=g) * 1.5 + 0.2).cuda()
    ga = torch.randn(t, c1, generator=g).cuda()
    gamma = (torch.rand(c1, generator=g) + 0.5)
    beta = torch.randn(c1, generator=g) * 0.3
    gamma[3] = -0.8                                                               # a negative gamma
    gamma[7], beta[7] = 0.01, -50.0                                               # a channel whose ReLU masks every token
    gamma, beta = gamma.cuda(), beta.cuda()
    w = (torch.randn(c1, 3 + 6, generator=g) * 0.3).cuda()
    z64 = z.double()
    mi = torch.cat([z64.mean(0), 1.0 / torch.sqrt(z64.var(0, unbiased=False) + 1e-5)]).float().contiguous()
    # fp64 statement: BatchNorm backward with the ReLU mask, coordinate-column gradients, scatter
    mu, istd, g64, b64 = mi[:c1].double(), mi[c1:].double(), gamma.double(), beta.double()
    xh = (z64 - mu) * istd
    dyh = torch.where(xh * g64 + b64 > 0, ga.double(), torch.zeros((), dtype=torch.float64, device="cuda"))
    assert not (xh[:, 7] * g64[7] + b64[7] > 0).any()
    gz = g64 * istd * (dyh - dyh.mean(0) - xh * (dyh * xh).mean(0))               # (t, c1)
    rel = torch.stack([xyz[i][idx[i].long()] for i in range(b)]).double() - new_xyz.double().unsqueeze(2)      # (b, m, ns, 3)
    gz4 = gz.view(b, m, ns, c1)
    want_dw = torch.einsum("bmso,bmsd->od", gz4, rel)
    want_new = -(gz4.sum(dim=2) @ w[:, :3].double())
    want_pts = torch.zeros(b, n, c1, dtype=torch.float64, device="cuda")
    for i in range(b):
        want_pts[i].index_add_(0, idx[i].reshape(-1).long(), gz4[i].reshape(m * ns, c1))
    want = {"g_pts": want_pts, "dw_xyz": want_dw, "grad_new_xyz": want_new, "dgamma": (dyh * xh).sum(0), "dbeta": dyh.sum(0)}
    inp = dict(b=b, n=n, m=m, ns=ns, c1=c1, xyz=xyz, new_xyz=new_xyz, idx=idx, z=z, ga=ga, gamma=gamma, beta=beta, w=w, mi=mi)
    # the three-kernel sequence this kernel replaces, on the same inputs: its errors are the yardstick
    gz1 = torch.empty_like(z)
    dg, db = torch.empty_like(gamma), torch.empty_like(beta)
    scratch = torch.empty((ext.bn_relu_scratch_bytes(c1),), dtype=torch.uint8, device="cuda")
    ext.bn_relu_bwd(z, ga, gamma, beta, mi, gz1, dg, db, scratch, t, c1)
    dw = torch.full_like(w, 7.0)
    gnew = torch.empty(b, m, 3, device="cuda")
    ext.sa_xyz_grad(gz1, xyz, new_xyz, idx, w, dw, gnew, b, n, m, ns, c1)
    pts = torch.zeros(b, n, c1, device="cuda")
    ext.group_rows_grad(b, n, c1, m * ns, gz1, idx, pts)
    base = {"g_pts": pts, "dw_xyz": dw[:, :3].clone(), "grad_new_xyz": gnew, "dgamma": dg, "dbeta": db}
    base_err = {k: (base[k].double() - want[k]).abs().max().item() for k in want}
    return inp, want, base_err


_CASES = {}


def _case(ns, c1, m):
    if (ns, c1, m) not in _CASES:
        _CASES[(ns, c1, m)] = _bwd_case(ns, c1, m)
    return _CASES[(ns, c1, m)]


def _run_fused(inp, with_new):
    from pdanet_amd import pointnet2_batch_cuda as ext
    b, n, m, ns, c1 = (inp[k] for k in ("b", "n", "m", "ns", "c1"))
    t = b * m * ns
    dg, db = torch.empty_like(inp["gamma"]), torch.empty_like(inp["beta"])
    sums = torch.empty(2 * c1, device="cuda")
    scratch = torch.empty((ext.bn_relu_scratch_bytes(c1),), dtype=torch.uint8, device="cuda")
    ga0 = inp["ga"].clone()
    ext.bn_relu_bwd_reduce(inp["z"], inp["ga"], inp["gamma"], inp["beta"], inp["mi"], dg, db, sums, scratch, t, c1)
    dw = torch.full_like(inp["w"], 7.0)
    gnew = torch.full((b, m, 3), float("nan"), device="cuda") if with_new else None
    pts = torch.full((b, n, c1), float("nan"), device="cuda")                     # the entry clears it
    ext.sa_point_grad_bn(inp["ga"], inp["z"], inp["mi"], inp["gamma"], inp["beta"], sums, inp["xyz"], inp["new_xyz"], inp["idx"], inp["w"],
                         dw, gnew, pts, b, n, m, ns, c1)
    assert torch.equal(inp["ga"], ga0)                                            # inputs are read only
    assert (dw[:, 3:] == 7.0).all()                                               # the feature columns are not this kernel's
    return {"g_pts": pts, "dw_xyz": dw[:, :3].clone(), "grad_new_xyz": gnew, "dgamma": dg, "dbeta": db}


@pytest.mark.parametrize("with_new", [True, False])
@pytest.mark.parametrize("ns,c1,m", [(3, 256, 8), (16, 256, 8), (3, 512, 8), (16, 512, 8), (3, 256, 300)])   # m = 300: 600 groups, more than the 512 workgroups
def test_point_grad_bn_against_fp64(ns, c1, m, with_new):
    """pda_bn_relu_bwd_reduce + pda_sa_point_grad_bn against an fp64 statement of BatchNorm backward with the ReLU mask, the
    coordinate-column gradients and the scatter.  The bound per output is twice the maximum error of the three-kernel sequence it
    replaces (pda_bn_relu_bwd, pda_sa_xyz_grad, fill + pda_group_rows_grad) against the same statement on the same inputs: the
    atomics arrive in another order and repeats are added in a register first, so last-bit differences are expected and more is a
    bug.  dgamma / dbeta come from the same reduction kernel and must be bit-equal to the sequence's.

    Maximum absolute errors measured on MI355X, three-kernel sequence -> fused (g_pts moves in its last bits from run to run
    on both sides: it is a sum of float atomics; the range over seven runs is given):
        (ns, c1, m)      g_pts                                  dw[:, 0:3]            grad_new_xyz
        (3, 256, 8)      5.3e-07..1.2e-06 -> 3.7e-07..4.9e-07   4.417e-06 -> same     7.179e-07 -> same
        (16, 256, 8)     1.2e-06..1.5e-06 -> 9.3e-07            1.188e-05 -> same     2.345e-06 -> same
        (3, 512, 8)      7.2e-07          -> 4.9e-07..9.0e-07   5.804e-06 -> same     1.187e-06 -> same
        (16, 512, 8)     1.1e-06..1.8e-06 -> 1.5e-06            1.676e-05 -> same     3.050e-06 -> same
        (3, 256, 300)    1.4e-05          -> 1.4e-05..1.7e-05   2.385e-05 -> same     1.527e-06 -> same
    (output scales 5..32, 56..296 and 8..38: one to two units in the last place throughout)."""
    inp, want, base_err = _case(ns, c1, m)
    got = _run_fused(inp, with_new)
    again = _run_fused(inp, with_new)
    for k in ("g_pts", "dw_xyz", "grad_new_xyz", "dgamma", "dbeta"):
        if got[k] is None:
            continue
        err = (got[k].double() - want[k]).abs().max().item()
        print("ns=%d c1=%d m=%d %-12s sequence %.3e fused %.3e (scale %.3e)" % (ns, c1, m, k, base_err[k], err, want[k].abs().max().item()))
        if k in ("dgamma", "dbeta"):
            assert err == base_err[k], k
        else:
            assert err <= 2.0 * base_err[k], k
    assert (got["g_pts"][:, 60:] == 0).all()                                      # a point no group references: exactly 0
    assert torch.isfinite(got["g_pts"]).all()
    assert torch.equal(got["dw_xyz"], again["dw_xyz"])                            # fixed-order sums
    if with_new:
        assert torch.equal(got["grad_new_xyz"], again["grad_new_xyz"])


def test_sa_wide_chain_fused_ends_equal_unfused_ends():
    """One iteration of SaWideChainTrain with PDA_SA_WIDE_FUSED_ENDS on against off at the smallest shape supported() takes
    (SA_WIDE_CHAIN_MIN_TOKENS = 32768 tokens, where pda_linear_wgrad_form(32768, 256, 256) == 2; B N = 4096 points for the split
    GEMM of the per-point projection): outputs and running statistics to 1e-6, input gradients to 2e-4 and parameter gradients to
    1e-3 of their scale (the bars of test_sa_wide_chain_equals_unfused_path)."""
    from pdanet_amd import pointnet2_utils as pu, synth
    B, N, M, ns, C = 2, 2048, 512, 32, 256
    assert B * M * ns == pu.SA_WIDE_CHAIN_MIN_TOKENS
    xyz = torch.from_numpy(synth.batch_xyz(B, N, config_id=6)).cuda()
    g = torch.Generator().manual_seed(21)
    ctr0 = (xyz[:, :M] + 0.05).contiguous()
    idx = pu.ball_query(8.4, ns, xyz, ctr0)
    feats0 = torch.randn(B, N, C, generator=g).cuda()
    layers = []
    for cin in (3 + C, 256, 256):
        layers += [torch.nn.Conv2d(cin, 256, 1, bias=False), torch.nn.BatchNorm2d(256), torch.nn.ReLU()]
    mlp0 = torch.nn.Sequential(*layers)
    with torch.no_grad():
        for mod in mlp0:
            if isinstance(mod, torch.nn.Conv2d):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * 0.05)
            elif isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(256, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(256, generator=g) * 0.2)
    res = {}
    try:
        for flag in (True, False):
            pu.SA_WIDE_FUSED_ENDS = flag
            mlp = copy.deepcopy(mlp0).cuda().train()
            ctr, feats = ctr0.clone().requires_grad_(True), feats0.clone().requires_grad_(True)
            assert pu.SaWideChainTrain.supported(xyz, ctr, feats, idx, mlp)
            out = pu.sa_wide_chain_train(xyz, ctr, feats, idx, mlp)
            out.pow(2).mean().backward()
            res[flag] = (out.detach(), feats.grad.clone(), ctr.grad.clone(), {k: p.grad.clone() for k, p in mlp.named_parameters()},
                         {k: v.clone() for k, v in mlp.state_dict().items() if "running" in k})
    finally:
        pu.SA_WIDE_FUSED_ENDS = True
    a, b = res[True], res[False]
    assert (a[0] - b[0]).abs().max().item() <= 1e-6 * max(1.0, b[0].abs().max().item())
    for k in b[4]:
        assert (a[4][k] - b[4][k]).abs().max().item() <= 1e-6 * max(1.0, b[4][k].abs().max().item()), k
    for i in (1, 2):
        assert (a[i] - b[i]).abs().max().item() <= 2e-4 * b[i].abs().max().item() + 1e-9
    gmax = max(float(v.abs().max()) for v in b[3].values())
    assert set(a[3]) == set(b[3]) and len(b[3]) == 9
    for k in b[3]:
        assert float((a[3][k] - b[3][k]).abs().max()) <= 1e-3 * float(b[3][k].abs().max()) + 1e-4 * gmax, k
