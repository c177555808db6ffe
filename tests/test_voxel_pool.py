"""csrc/voxel_pool.hip (pda_voxel_pool_moments / _fwd / _bwd) against float64 statements in plain numpy and torch on the CPU.

The statements follow the kernel file's contract: a slot reads nothing (rel = 0, f = 0) when its row is empty (first slot < 0)
or its index lies outside [0, N); rel is the float32 difference; value = relu(f + scale * (w . rel) + shift); out is the
row's largest value and arg the first slot that attains it.

Shapes: M = 1, 63, 64, 65, 257 (one point, one short of / exactly / one past the 64 points of eight C = 32 workgroup rows,
several workgroups with a ragged tail), nsample 1 and 16, N = 1 and 200, C = 32 and 64 (the two kernels).

Mutation record (scratch copies of voxel_pool.hip, each built into a library of its own and run through this file on an
MI355X; the real library passes all 23 GPU tests):
  * last maximum instead of first (`v >= best`, the padded-duplicate skip removed): test_forward_exact (all four cases) and
    test_bad_indices_write_nothing_out_of_bounds (both) fail on arg; 6 failures.
  * empties not zeroed (vp_row without the empty-row rule, all slots of an empty row walked): test_moments (0.2 and 1.0 empty,
    ns = 16), test_forward_exact (4), test_forward_normal (2), test_backward (the six ns = 16 cases),
    test_empty_rows_give_no_feature_gradient_but_count_in_dbeta and test_bad_indices_write_nothing_out_of_bounds (2) fail; 17.
  * n counted without the padded slots (the moments kernel skips a padded duplicate of slot 0): test_moments (0.0 and 0.2
    empty, ns = 16), test_backward (M = 63 and 257 with ns = 16, through the statistics) and
    test_bad_indices_write_nothing_out_of_bounds (2) fail; 8.
Largest observed error over bound on the MI355X: moments 0.029; forward |out - ref| 0.222, fp64 maximum against the value at
the device's arg 0.000 (no near-tie flipped); grad_features_in 0.162; dW / dgamma / dbeta at most 8.6e-8 / 9.1e-8 / 5.2e-8
against 1.0e-7 .. 2.4e-6 / 9.3e-8 .. 1.6e-7 / 5.6e-8 .. 1.2e-7 for the float32 composition on the CPU."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
F32, I32 = np.float32, np.int32
MS = [1, 63, 64, 65, 257]
U24, U53 = 2.0 ** -24, 2.0 ** -53


def make_idx(rng, M, ns, N, empty_share):
    """(M, ns) int32 in the voxel query's form: cnt distinct hits, then the first hit repeated; -1 then zeros when empty."""
    idx = np.zeros((M, ns), I32)
    for m in range(M):
        if rng.random() < empty_share:
            idx[m, 0] = -1
            continue
        cnt = int(rng.integers(1, min(ns, N) + 1))
        hits = rng.choice(N, cnt, replace=False)
        idx[m] = hits[0]
        idx[m, :cnt] = hits
    return idx


def lattice(rng, n, lo=-16, hi=17):
    return (rng.integers(lo, hi, (n, 3)) / 8).astype(F32)


def rel_of(idx, xyz, new_xyz):
    """float32 rel (M, ns, 3) with the slots that read nothing at 0, and the mask of the slots that read a row"""
    N = xyz.shape[0]
    reads = (idx[:, :1] >= 0) & (idx >= 0) & (idx < N)
    g = np.where(reads, idx, 0)
    rel = (xyz[g] - new_xyz[:, None, :]).astype(F32)
    rel[~reads] = 0
    return rel, reads, g


def values64(feat, idx, xyz, new_xyz, w, scale, shift):
    """-> v (M, ns, C) float64 = relu(f + scale * (w . rel) + shift), terms (M, ns, C) = |f| + sum_i |scale w_i x_i| + |shift|"""
    rel, reads, g = rel_of(idx, xyz, new_xyz)
    f = np.where(reads[..., None], feat[g], 0).astype(np.float64)
    prod = scale.astype(np.float64)[None, None, :, None] * w.astype(np.float64)[None, None] * rel.astype(np.float64)[:, :, None, :]
    v = np.maximum(f + prod.sum(-1) + shift.astype(np.float64), 0)
    return v, np.abs(f) + np.abs(prod).sum(-1) + np.abs(shift.astype(np.float64))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- 1. moments -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ns", [1, 16])
@pytest.mark.parametrize("empty_share", [0.0, 0.2, 1.0])
def test_moments(ns, empty_share):
    from pdanet_amd.voxel_pool_modules import voxel_pool_moments
    worst = 0.0
    for M in MS:
        rng = np.random.default_rng(1000 * M + ns)
        N = 200
        xyz, new_xyz = rng.standard_normal((N, 3)).astype(F32), rng.standard_normal((M, 3)).astype(F32)
        idx = make_idx(rng, M, ns, N, empty_share)
        if empty_share == 0.2 and M > 1:
            idx[-1] = [N + 3] + [0] * (ns - 1)                   # a first slot past N: that slot reads nothing, the rest do
        rel = rel_of(idx, xyz, new_xyz)[0].astype(np.float64).reshape(-1, 3)
        x, y, z = rel[:, 0], rel[:, 1], rel[:, 2]
        terms = np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z])
        got = voxel_pool_moments(dev(idx), dev(xyz), dev(new_xyz)).cpu().numpy()
        bound = M * ns * U53 * np.abs(terms).sum(axis=1)
        err = np.abs(got - terms.sum(axis=1))
        assert (err <= bound).all(), (M, ns, err, bound)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        if ns > 1 and empty_share == 0.0:
            assert (idx[:, 1:] == idx[:, :1]).any()              # padded duplicates are in the sums
    print("moments ns=%d empty=%.1f: largest error / bound %.3f" % (ns, empty_share, worst))


# ---- 2. forward on exact data ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("N", [1, 200])
def test_forward_exact(C, N):
    from pdanet_amd.voxel_pool_modules import voxel_pool_fwd
    ties = 0
    for M in MS:
        for ns in (1, 16):
            rng = np.random.default_rng(M * 100 + ns + C)
            xyz, new_xyz = lattice(rng, N), lattice(rng, M)
            idx = make_idx(rng, M, ns, N, 0.2)
            feat = rng.integers(-1, 2, (N, C)).astype(F32)
            if N > 8:
                feat[1::2] = feat[0::2]                          # equal rows: ties between different voxels ...
            w = rng.integers(-2, 3, (C, 3)).astype(F32)
            w[C // 2:] = 0                                       # ... which the position term does not break here
            shift = rng.integers(-2, 3, C).astype(F32)
            scale = np.ones(C, F32)
            v, _ = values64(feat, idx, xyz, new_xyz, w, scale, shift)
            out, arg = voxel_pool_fwd(dev(feat), dev(idx), dev(xyz), dev(new_xyz), dev(w), dev(scale), dev(shift))
            assert np.array_equal(out.cpu().numpy().astype(np.float64), v.max(axis=1)), (M, ns)
            assert np.array_equal(arg.cpu().numpy(), v.argmax(axis=1).astype(np.uint8)), (M, ns)      # argmax: the first maximum
            ties += int(((v == v.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    assert ties > 0


# ---- 3. forward on normal data --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", [32, 64])
def test_forward_normal(C):
    from pdanet_amd.voxel_pool_modules import voxel_pool_fwd
    worst = [0.0, 0.0]
    for M in MS:
        for ns in (1, 16):
            rng = np.random.default_rng(M * 7 + ns + C)
            N = 200
            xyz, new_xyz = rng.standard_normal((N, 3)).astype(F32), rng.standard_normal((M, 3)).astype(F32)
            idx = make_idx(rng, M, ns, N, 0.2)
            feat = rng.standard_normal((N, C)).astype(F32)
            w, shift = rng.standard_normal((C, 3)).astype(F32), rng.standard_normal(C).astype(F32)
            scale = (rng.random(C) + 0.5).astype(F32)
            v, terms = values64(feat, idx, xyz, new_xyz, w, scale, shift)
            out, arg = voxel_pool_fwd(dev(feat), dev(idx), dev(xyz), dev(new_xyz), dev(w), dev(scale), dev(shift))
            out, arg = out.cpu().numpy().astype(np.float64), arg.cpu().numpy().astype(np.int64)
            assert (arg < ns).all()
            at = np.take_along_axis(v, arg[:, None, :], axis=1)[:, 0]
            bound = 13 * U24 * np.take_along_axis(terms, arg[:, None, :], axis=1)[:, 0]
            assert (np.abs(out - at) <= bound).all(), (M, ns)
            assert (v.max(axis=1) - at <= 2 * bound).all(), (M, ns)
            worst[0] = max(worst[0], float((np.abs(out - at) / bound).max()))
            worst[1] = max(worst[1], float(((v.max(axis=1) - at) / (2 * bound)).max()))
    print("forward C=%d: largest |out - ref| / bound %.3f, largest (max - value at arg) / bound %.3f" % (C, worst[0], worst[1]))


# ---- 4. backward against float64 autograd ---------------------------------------------------------------------------------
def composition(dtype, feat, idx, xyz, new_xyz, w, gamma, beta, eps, arg, grad_out):
    """BatchNorm2d in training mode over all M * ns slots, the max replaced by a gather at `arg`; -> gradients, out"""
    rel, reads, g = rel_of(idx, xyz, new_xyz)
    t = lambda a: torch.tensor(a, dtype=dtype)
    feat, w, gamma, beta = (t(a).requires_grad_(True) for a in (feat, w, gamma, beta))
    y = t(rel) @ w.t()                                                            # (M, ns, C)
    flat = y.reshape(-1, y.shape[-1])
    mean, var = flat.mean(dim=0), flat.var(dim=0, unbiased=False)
    z = (y - mean) / torch.sqrt(var + eps) * gamma + beta
    f = feat[torch.from_numpy(g).long()] * t(reads[..., None].astype(np.float64))
    v = torch.relu(f + z)
    out = torch.gather(v, 1, torch.from_numpy(arg.astype(np.int64))[:, None, :])[:, 0]
    (out * t(grad_out)).sum().backward()
    return [a.grad.numpy().astype(np.float64) for a in (feat, w, gamma, beta)], out.detach().numpy()


def rel_err(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


@gpu
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("M,ns", [(1, 16), (63, 16), (65, 1), (257, 16)])
def test_backward(C, M, ns):
    from pdanet_amd.voxel_pool_modules import _FusedVoxelPool
    rng = np.random.default_rng(M + ns + C)
    N, eps = 120, 1e-5
    xyz, new_xyz = rng.standard_normal((N, 3)).astype(F32), rng.standard_normal((M, 3)).astype(F32)
    idx = make_idx(rng, M, ns, N, 0.2)
    idx[0, 0] = -1                                                                # at least one empty row
    idx[0, 1:] = 0
    feat = rng.standard_normal((N, C)).astype(F32)
    w, beta = rng.standard_normal((C, 3)).astype(F32), (rng.standard_normal(C) * 0.5).astype(F32)
    gamma = (rng.random(C) + 0.5).astype(F32)
    grad_out = rng.standard_normal((M, C)).astype(F32)
    conv = torch.nn.Conv2d(3, C, kernel_size=1, bias=False).cuda()
    bn = torch.nn.BatchNorm2d(C, eps=eps).cuda().train()
    with torch.no_grad():
        conv.weight.copy_(dev(w).view(C, 3, 1, 1)); bn.weight.copy_(dev(gamma)); bn.bias.copy_(dev(beta))
    f_dev = dev(feat).requires_grad_(True)
    out, arg = _FusedVoxelPool.apply(f_dev, dev(idx), dev(xyz), dev(new_xyz), conv.weight, bn.weight, bn.bias, bn, True)
    (out * dev(grad_out)).sum().backward()
    arg = arg.cpu().numpy()
    got = [f_dev.grad.cpu().numpy(), conv.weight.grad.view(C, 3).cpu().numpy(), bn.weight.grad.cpu().numpy(), bn.bias.grad.cpu().numpy()]
    ref, out64 = composition(torch.float64, feat, idx, xyz, new_xyz, w, gamma, beta, eps, arg, grad_out)
    c32, _ = composition(torch.float32, feat, idx, xyz, new_xyz, w, gamma, beta, eps, arg, grad_out)

    # the feature gradient: every element is a sum of k incoming gradients
    rel, reads, g = rel_of(idx, xyz, new_xyz)
    live = (out64 > 0) & np.take_along_axis(reads, arg.astype(np.int64), axis=1)
    rows = np.take_along_axis(g, arg.astype(np.int64), axis=1)                    # (M, C)
    k, mag = np.zeros((N, C)), np.zeros((N, C))
    cols = np.broadcast_to(np.arange(C), (M, C))
    np.add.at(k, (rows[live], cols[live]), 1)
    np.add.at(mag, (rows[live], cols[live]), np.abs(grad_out.astype(np.float64))[live])
    bound = (k + 8) * U24 * mag
    err = np.abs(got[0] - ref[0])
    assert (err <= bound).all(), float((err - bound).max())
    figures = ["grad_features_in: largest error / bound %.3f" % float((err / np.maximum(bound, 1e-300)).max())]
    for name, a, r, c in zip(("dW", "dgamma", "dbeta"), got[1:], ref[1:], c32[1:]):
        e_dev, e_f32 = rel_err(a, r), rel_err(c, r)
        figures.append("%s: device %.2e, float32 CPU %.2e" % (name, e_dev, e_f32))
        assert e_dev <= 4 * e_f32, (name, e_dev, e_f32)
    print("backward C=%d M=%d ns=%d: " % (C, M, ns) + "; ".join(figures))
    # running statistics: BatchNorm2d's update with the unbiased variance over n = M * ns slots
    y = rel.astype(np.float64).reshape(-1, 3) @ w.astype(np.float64).T
    n = M * ns
    assert np.allclose(bn.running_mean.cpu().numpy(), 0.1 * y.mean(0), rtol=1e-5, atol=1e-7)
    assert np.allclose(bn.running_var.cpu().numpy(), 0.9 + 0.1 * y.var(0) * n / max(n - 1, 1), rtol=1e-5, atol=1e-7)
    assert int(bn.num_batches_tracked) == 1


@gpu
def test_empty_rows_give_no_feature_gradient_but_count_in_dbeta():
    from pdanet_amd.voxel_pool_modules import voxel_pool_bwd, voxel_pool_fwd
    rng = np.random.default_rng(5)
    M, ns, N, C = 65, 16, 10, 32
    idx = np.zeros((M, ns), I32)
    idx[:, 0] = -1
    xyz, new_xyz = lattice(rng, N), lattice(rng, M)
    feat = rng.standard_normal((N, C)).astype(F32)
    w = rng.standard_normal((C, 3)).astype(F32)
    shift = np.where(np.arange(C) % 2 == 0, 1.0, -1.0).astype(F32)              # relu(shift): every other channel is live
    grad_out = rng.standard_normal((M, C)).astype(F32)
    args = (dev(idx), dev(xyz), dev(new_xyz), dev(w))
    out, arg = voxel_pool_fwd(dev(feat), *args, dev(np.ones(C, F32)), dev(shift))
    assert np.array_equal(out.cpu().numpy(), np.broadcast_to(np.maximum(shift, 0), (M, C))) and int(arg.max()) == 0
    grad_feat, win = voxel_pool_bwd(dev(grad_out), out, arg, *args, N)
    assert not grad_feat.any()
    want = np.where(shift > 0, grad_out.astype(np.float64).sum(axis=0), 0)
    assert np.abs(win[0].cpu().numpy() - want).max() <= M * U53 * np.abs(grad_out).sum(axis=0).max()
    assert not win[1:].any()                                                      # rel* = 0 in every row


# ---- 5. bad indices -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", [32, 64])
def test_bad_indices_write_nothing_out_of_bounds(C):
    """Every output buffer sits between guard rows; the entries get pointers into the middle."""
    from pdanet_amd import _lib
    from pdanet_amd.pointnet2_batch_cuda import _call
    rng = np.random.default_rng(9)
    M, ns, N, G = 65, 16, 50, 4
    idx = make_idx(rng, M, ns, N, 0.3)
    idx[1] = [N] + [N + 7] * (ns - 1)                     # past the end, first slot included
    idx[2, 3:] = [2 ** 31 - 1, -5, N, -2 ** 31] + [idx[2, 0]] * (ns - 7)
    idx[3] = [-1] + [N + 1] * (ns - 1)                    # an empty row whose other slots are bad as well
    xyz, new_xyz = lattice(rng, N), lattice(rng, M)
    feat = rng.integers(-2, 3, (N, C)).astype(F32)
    w, shift = rng.integers(-2, 3, (C, 3)).astype(F32), rng.integers(-1, 2, C).astype(F32)
    scale = np.ones(C, F32)
    grad_out = rng.integers(-2, 3, (M, C)).astype(F32)
    d_idx, d_xyz, d_new, d_feat, d_w, d_scale, d_shift, d_grad = (dev(a) for a in (idx, xyz, new_xyz, feat, w, scale, shift, grad_out))
    need = int(_lib.load().pda_voxel_pool_scratch_doubles(M, C, ns))
    out = torch.full((M + 2 * G, C), 777.0, device="cuda")
    arg = torch.full((M + 2 * G, C), 201, dtype=torch.uint8, device="cuda")
    grad_feat = torch.full((N + 2 * G, C), 777.0, device="cuda")
    grad_feat[G:G + N] = 0
    scratch = torch.full((need + 2 * G,), 777.0, dtype=torch.float64, device="cuda")
    sums = torch.full((9 + 2 * G,), 777.0, dtype=torch.float64, device="cuda")
    win = torch.full((5 * C + 2 * G,), 777.0, dtype=torch.float64, device="cuda")
    _call("pda_voxel_pool_moments", d_idx, d_idx.data_ptr(), d_xyz.data_ptr(), d_new.data_ptr(), scratch[G:].data_ptr(),
          sums[G:].data_ptr(), N, M, ns)
    _call("pda_voxel_pool_fwd", d_idx, d_feat.data_ptr(), d_idx.data_ptr(), d_xyz.data_ptr(), d_new.data_ptr(), d_w.data_ptr(),
          d_scale.data_ptr(), d_shift.data_ptr(), out[G:].data_ptr(), arg[G:].data_ptr(), N, M, C, ns)
    _call("pda_voxel_pool_bwd", d_idx, d_grad.data_ptr(), out[G:].data_ptr(), arg[G:].data_ptr(), d_idx.data_ptr(), d_xyz.data_ptr(),
          d_new.data_ptr(), d_w.data_ptr(), grad_feat[G:].data_ptr(), scratch[G:].data_ptr(), win[G:].data_ptr(), N, M, C, ns)
    torch.cuda.synchronize()
    for name, buf, rows in (("out", out, M), ("arg", arg, M), ("grad_features_in", grad_feat, N), ("scratch", scratch, need),
                            ("sums", sums, 9), ("winner sums", win, 5 * C)):
        guard = torch.cat([buf[:G].reshape(-1), buf[G + rows:].reshape(-1)]).double()
        assert bool((guard == (201 if buf.dtype == torch.uint8 else 777)).all()), name
    v, _ = values64(feat, idx, xyz, new_xyz, w, scale, shift)
    assert np.array_equal(out[G:G + M].cpu().numpy().astype(np.float64), v.max(axis=1))
    assert np.array_equal(arg[G:G + M].cpu().numpy(), v.argmax(axis=1).astype(np.uint8))
    rel, reads, g = rel_of(idx, xyz, new_xyz)
    a = v.argmax(axis=1)
    live = (v.max(axis=1) > 0) & np.take_along_axis(reads, a, axis=1)
    want = np.zeros((N, C))
    np.add.at(want, (np.take_along_axis(g, a, axis=1)[live], np.broadcast_to(np.arange(C), (M, C))[live]), grad_out.astype(np.float64)[live])
    assert np.array_equal(grad_feat[G:G + N].cpu().numpy().astype(np.float64), want)          # small integers: exact in any order
    relf = rel.astype(np.float64).reshape(-1, 3)
    assert np.array_equal(sums[G:G + 3].cpu().numpy(), relf.sum(axis=0))


def test_sizes_are_refused_before_any_launch():
    import ctypes
    from pdanet_amd import _lib
    lib = _lib.load()
    assert lib.pda_voxel_pool_scratch_doubles(100, 48, 16) == -1 and lib.pda_voxel_pool_scratch_doubles(100, 32, 256) == -1
    assert lib.pda_voxel_pool_scratch_doubles(55296, 32, 16) >= 9
    assert lib.pda_voxel_pool_fwd(None, None, None, None, None, None, None, None, None, 10, 10, 48, 16, None) == 1
    assert b"pda_voxel_pool_fwd" in lib.pda_last_error()
    assert lib.pda_voxel_pool_fwd(None, None, None, None, None, None, None, None, None, 10, 0, 32, 16, None) == 0      # no points
    assert lib.pda_voxel_pool_bwd(None, None, None, None, None, None, None, None, None, None, 10, 10, 32, 0, None) == 1
    assert lib.pda_voxel_pool_moments(None, None, None, None, ctypes.c_void_p(8), 10, 10, 16, None) == 1 and b"null" in lib.pda_last_error()
