"""The contract of the sparse 3D convolutions restated with dense library calls on the CPU: features
scattered into a dense float64 grid, torch.nn.functional.conv3d over it, and the same convolution of the occupancy with a
kernel of ones (> 0 => active) for the output sites of a strided convolution.  Rows come back in ascending linear key
((b * D' + z) * H' + y) * W' + x (a submanifold convolution keeps the input's rows and their order).  Autograd through
these calls gives the reference gradients.  rulebook() restates the index stage with a dictionary of sites.  dense_run()
walks a module tree of sparse layers (by class name and attributes only) and evaluates it densely: the whole-stack
reference of the backbones.  None of this uses the code under test."""
import itertools

import numpy as np
import torch
import torch.nn.functional as F


def triple(v):
    return tuple(int(x) for x in v) if isinstance(v, (list, tuple)) else (int(v),) * 3


def out_shape(shape, k, s, p):
    return [(int(i) + 2 * pp - kk) // ss + 1 for i, kk, ss, pp in zip(shape, k, s, p)]


def linear_key(idx, shape):
    idx = np.asarray(idx, np.int64)
    return ((idx[:, 0] * shape[0] + idx[:, 1]) * shape[1] + idx[:, 2]) * shape[2] + idx[:, 3]


def scatter_dense(features, indices, shape, batch):
    """features (N, C) tensor, indices (N, 4) -> (B, C, D, H, W), zero elsewhere (index_put; differentiable)."""
    idx = torch.as_tensor(np.asarray(indices, np.int64))
    dense = features.new_zeros((batch, shape[0], shape[1], shape[2], features.shape[1]))
    dense = dense.index_put((idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]), features)
    return dense.permute(0, 4, 1, 2, 3)


def occupancy(indices, shape, batch):
    return scatter_dense(torch.ones((len(indices), 1), dtype=torch.float64), indices, shape, batch)


def output_sites(indices, shape, batch, k, s, p):
    """(out_indices (M, 4) int64 in ascending key order, output shape) of a strided convolution."""
    k, s, p = triple(k), triple(s), triple(p)
    occ = F.conv3d(occupancy(indices, shape, batch), torch.ones((1, 1) + k, dtype=torch.float64), stride=s, padding=p)
    return torch.nonzero(occ[:, 0] > 0).numpy(), list(occ.shape[2:])


def conv_rows(features, indices, shape, batch, weight, bias, k, s, p, subm):
    """The convolution's output rows.  features (N, C_in), weight (C_out, kD, kH, kW, C_in) (spconv 2.x layout), bias (C_out)
    or None, any float dtype -> (out_rows (M, C_out), out_indices (M, 4) int64, output shape)."""
    k, s, p = triple(k), triple(s), triple(p)
    if subm:
        s, p = (1, 1, 1), tuple(v // 2 for v in k)
    dense = F.conv3d(scatter_dense(features, indices, shape, batch), weight.permute(0, 4, 1, 2, 3), None, stride=s, padding=p)
    if subm:
        sites, oshape = np.asarray(indices, np.int64), list(shape)
    else:
        sites, oshape = output_sites(indices, shape, batch, k, s, p)
    st = torch.as_tensor(sites)
    rows = dense.permute(0, 2, 3, 4, 1)[st[:, 0], st[:, 1], st[:, 2], st[:, 3]]
    if bias is not None:
        rows = rows + bias
    return rows, sites, oshape


def rulebook(indices, shape, batch, k, s, p, subm):
    """(out_indices (M, 4), nbr_out (M, T), nbr_in (N, T)) int32 from a dictionary of sites; taps t = (tz * kH + ty) * kW + tx."""
    k, s, p = triple(k), triple(s), triple(p)
    indices = np.asarray(indices, np.int64)
    if subm:
        s, p = (1, 1, 1), tuple(v // 2 for v in k)
        sites, oshape = indices, list(shape)
    else:
        sites, oshape = output_sites(indices, shape, batch, k, s, p) if len(indices) else (np.zeros((0, 4), np.int64), out_shape(shape, k, s, p))
    row_of = {tuple(c): i for i, c in enumerate(indices.tolist())}
    out_of = {tuple(c): i for i, c in enumerate(sites.tolist())}
    taps = list(itertools.product(range(k[0]), range(k[1]), range(k[2])))
    nbr_out = np.full((len(sites), len(taps)), -1, np.int32)
    nbr_in = np.full((len(indices), len(taps)), -1, np.int32)
    for o, (b, z, y, x) in enumerate(sites.tolist()):
        for t, (tz, ty, tx) in enumerate(taps):
            site = (b, z * s[0] - p[0] + tz, y * s[1] - p[1] + ty, x * s[2] - p[2] + tx)      # outside the grid: not a key
            j = row_of.get(site, -1)
            nbr_out[o, t] = j
            if j >= 0:
                nbr_in[j, t] = o
    return sites.astype(np.int32), nbr_out, nbr_in


def reference(features, indices, shape, batch, weight, bias, grad_out_of, k, s, p, subm):
    """Forward rows and the gradients of sum(rows * grad_out) in float64.  grad_out_of(M) -> (M, C_out) array.  Also S (the
    sums of |a * b| behind every element) and P (their number of products), from the same calls on absolute values and on
    ones.  Returns a dict of numpy float64 arrays: out, g_feat, g_w, g_b, and S_*/P_* alike."""
    def run(f, w, b, go):
        f = torch.tensor(np.asarray(f, np.float64), requires_grad=True)
        w = torch.tensor(np.asarray(w, np.float64), requires_grad=True)
        b = None if b is None else torch.tensor(np.asarray(b, np.float64), requires_grad=True)
        rows, sites, oshape = conv_rows(f, indices, shape, batch, w, b, k, s, p, subm)
        g = torch.tensor(np.asarray(go(len(sites)) if callable(go) else go, np.float64))
        if len(sites) and len(indices):
            (rows * g).sum().backward()
        z = lambda t: None if t is None else (np.zeros(t.shape) if t.grad is None else t.grad.numpy())
        return rows.detach().numpy(), z(f), z(w), z(b), sites, oshape, g.numpy()

    out, g_feat, g_w, g_b, sites, oshape, go = run(features, weight, bias, grad_out_of)
    ab = lambda a: None if a is None else np.abs(np.asarray(a, np.float64))
    on = lambda a: None if a is None else np.ones_like(np.asarray(a, np.float64))
    S = run(ab(features), ab(weight), ab(bias), ab(go))
    P = run(on(features), on(weight), on(bias), on(go))
    return dict(out=out, g_feat=g_feat, g_w=g_w, g_b=g_b, sites=sites, out_shape=oshape, grad_out=go,
                S_out=S[0], S_feat=S[1], S_w=S[2], S_b=S[3], P_out=P[0], P_feat=P[1], P_w=P[2], P_b=P[3])


# ---- a whole stack, densely ----------------------------------------------------------------------------------------------
class DenseSparse:
    """A sparse tensor held densely: values (B, C, D, H, W), zero off the active sites, and mask (B, D, H, W) bool."""

    def __init__(self, values, mask):
        self.values, self.mask = values, mask

    def rows(self):
        return self.values.permute(0, 2, 3, 4, 1)[self.mask]          # ascending key order

    def with_rows(self, rows):
        v = self.values.new_zeros(self.values.permute(0, 2, 3, 4, 1).shape[:4] + (rows.shape[1],))
        v = v.masked_scatter(self.mask.unsqueeze(-1), rows) if rows.numel() else v
        return DenseSparse(v.permute(0, 4, 1, 2, 3), self.mask)


def dense_input(features, indices, shape, batch):
    return DenseSparse(scatter_dense(features, indices, shape, batch), occupancy(indices, shape, batch)[:, 0] > 0)


def dense_run(module, x):
    """Evaluates a tree of sparse layers densely.  Dispatch is by class name: SparseSequential and the backbones' blocks are
    walked; a SubMConv3d / SparseConv3d is F.conv3d with its weight (C_out, kD, kH, kW, C_in) and the occupancy rule;
    BatchNorm1d and ReLU act on the active rows (the module itself is called: plain torch)."""
    name = type(module).__name__
    if name == 'SparseSequential':
        for child in module._modules.values():
            x = dense_run(child, x)
        return x
    if name in ('SubMConv3d', 'SparseConv3d'):
        k, w = module.kernel_size, module.weight
        s, p = ((1, 1, 1), tuple(v // 2 for v in k)) if module.subm else (module.stride, module.padding)
        v = F.conv3d(x.values, w.permute(0, 4, 1, 2, 3), module.bias, stride=s, padding=p)
        if module.subm:
            mask = x.mask
        else:
            occ = F.conv3d(x.mask.unsqueeze(1).to(torch.float64), torch.ones((1, 1) + tuple(k), dtype=torch.float64), stride=s, padding=p)
            mask = occ[:, 0] > 0
        return DenseSparse(v * mask.unsqueeze(1).to(v.dtype), mask)
    if name == 'SparseBasicBlock':
        out = dense_run(module.conv1, x)
        out = out.with_rows(module.relu(module.bn1(out.rows())))
        out = dense_run(module.conv2, out)
        out = out.with_rows(module.bn2(out.rows()))
        assert module.downsample is None
        return out.with_rows(module.relu(out.rows() + x.rows()))
    return x.with_rows(module(x.rows()))                               # BatchNorm1d, ReLU


def dense_backbone(model, features, indices, batch):
    """VoxelBackBone8x / VoxelResBackBone8x densely: {'x_conv1'..'x_conv4', 'out'} -> DenseSparse."""
    x = dense_run(model.conv_input, dense_input(features, indices, model.sparse_shape, batch))
    res = {}
    for i in (1, 2, 3, 4):
        x = dense_run(getattr(model, 'conv%d' % i), x)
        res['x_conv%d' % i] = x
    res['out'] = dense_run(model.conv_out, x)
    return res
