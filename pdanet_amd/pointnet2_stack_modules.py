"""StackSAModuleMSG and build_local_aggregation_module (pcdet/ops/pointnet2/pointnet2_stack/pointnet2_modules.py:10-112):
the set-abstraction layer of VoxelSetAbstraction and of PVRCNNHead's RoI-grid pool, under the reference's constructor, module
names (groupers, mlps) and state-dict keys.  The constructor copies its `mlps` argument and build_local_aggregation_module
copies config.MLPS: the reference prepends the input channels (and adds 3) in place, this leaves the model config as it was.

Two paths compute one scale, chosen when the layer runs by PDA_STACK_SA = fused | composed:
  composed  the reference's sequence over QueryAndGroup and torch modules.  Serves every configuration.
  fused     csrc/stack_sa.hip, the default where it applies: exactly two Conv-BN-ReLU layers, max_pool, use_xyz, features
            given, both widths in {16, 32, 64}, nsample <= 255.  The ball query's idx goes straight into the kernels; no
            (M x nsample)-sized tensor is made in the forward, and one (e1) in the backward.

The fused scale.  The first conv is split W1 = [W1x | W1f] (xyz first, as QueryAndGroup concatenates): F = features W1f^T is an
ordinary matmul over the N source rows and autograd carries dW1f and dfeatures from dF.  The kernels make y1 = F[g] + W1x rel,
z1 = relu(s1 y1 + t1), y2 = W2 z1 per slot and keep per (centre, channel) the extreme of y2 that the sign of the second
BatchNorm's weight selects (a max over relu(s2 y2 + t2) is attained at the largest y2 where s2 >= 0, at the smallest
otherwise).  BatchNorm2d's statistics over all n = M nsample slots -- padded repeats and empty rows included, as the reference's
zeroed grouped tensor has them -- come from float64 sums the kernels leave; this module finishes them in float64, updates
running_mean / running_var (unbiased) / num_batches_tracked as nn.BatchNorm2d does, and in eval mode uses the running
statistics.  The backward is closed form (`bn_backward_constants`): with e the gradient at a BatchNorm's output,
    dbeta = sum e,   dgamma = (sum e y - mean sum e) istd,   dy = s e - A - B y,
    A = s (dbeta / n - mean istd dgamma / n),   B = s istd dgamma / n       (A = B = 0 with running statistics)
so two recompute passes over the slots suffice.  Everything but dF (float atomics) is identical from run to run.

xyz and new_xyz receive NO gradient on the fused path: in PV-RCNN they are raw points, voxel centres and the grid points of
detached RoIs.  (The composed path differentiates rel as the reference does.)  dF is added with float atomics, so dfeatures and
the feature columns of the first conv's weight gradient, which autograd derives from it, are not bit-reproducible.

Out of scope: VectorPoolAggregationModuleMSG (PV-RCNN++), StackPointnetFPModule."""
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import pointnet2_stack_cuda as pointnet2
from . import pointnet2_stack_utils as pointnet2_utils
from ._lib import load as _load
from .config import fused_or_composed
from .pointnet2_batch_cuda import F32, I32, _call, _chk

# 'fused' (default) or 'composed', read when a layer runs
ENV = "PDA_STACK_SA"
sa_path = partial(fused_or_composed, ENV)
FUSED_CHANNELS = (16, 32, 64)
FUSED_MAX_NSAMPLE = 255
U8, F64 = torch.uint8, torch.float64


# ---- the float64 finish: plain torch, any device --------------------------------------------------------------------------
def batch_moments(sums, n):
    """sums (2, C) float64 [sum y, sum y^2] over n slots -> (mean, biased var) float64."""
    mean = sums[0] / n
    return mean, (sums[1] / n - mean * mean).clamp(min=0)


def bn_scale_shift(gamma, beta, mean, var, eps):
    """-> (s, t, istd) float64 with BatchNorm(y) = s y + t."""
    istd = 1.0 / torch.sqrt(var + eps)
    s = gamma.double() * istd
    return s, beta.double() - mean * s, istd


def bn_backward_constants(sum_e, sum_ey, s, mean, istd, n, batch_stats):
    """sum e and sum e y per channel -> (dgamma, dbeta, A, B) float64 of dy = s e - A - B y."""
    dbeta = sum_e
    dgamma = (sum_ey - mean * sum_e) * istd
    if not batch_stats:
        return dgamma, dbeta, torch.zeros_like(s), torch.zeros_like(s)
    b = s * istd * dgamma / n
    return dgamma, dbeta, s * dbeta / n - mean * b, b


def _statistics(bn, sums, n, training):
    """The (mean, var) a BatchNorm normalises with, and whether they are the batch's; updates the buffers in training."""
    batch_stats = training or bn.running_mean is None
    if not batch_stats:
        return bn.running_mean.double(), bn.running_var.double(), False
    mean, var = batch_moments(sums, n)
    if training and bn.running_mean is not None:
        bn.num_batches_tracked += 1
        mom = bn.momentum if bn.momentum is not None else 1.0 / bn.num_batches_tracked.double()
        unbiased = var * (n / max(n - 1, 1))
        bn.running_mean.mul_(1 - mom).add_((mom * mean).to(bn.running_mean.dtype))
        bn.running_var.mul_(1 - mom).add_((mom * unbiased).to(bn.running_var.dtype))
    return mean, var, True


# ---- the entry points of csrc/stack_sa.hip --------------------------------------------------------------------------------
def _scratch(m, c1, c2, ns, device):
    need = _load().pda_stack_sa_scratch_doubles(m, c1, c2, ns)
    if need < 0:
        raise ValueError("stack sa: m=%d c1=%d c2=%d nsample=%d is outside the fused kernels (widths 16, 32 or 64, nsample "
                         "1..255)" % (m, c1, c2, ns))
    return torch.empty((max(int(need), 1),), dtype=F64, device=device)


class _Geometry:
    """What every entry reads: F, xyz, new_xyz, the two count vectors and idx, checked once."""

    def __init__(self, f, xyz, new_xyz, xyz_batch_cnt, new_xyz_batch_cnt, idx):
        self.n, self.c1 = f.shape
        self.m, self.ns = idx.shape
        self.b = xyz_batch_cnt.shape[0]
        if xyz.shape != (self.n, 3) or new_xyz.shape != (self.m, 3) or new_xyz_batch_cnt.shape[0] != self.b:
            raise ValueError("stack sa: shapes disagree")
        self.device = idx.device
        self.first = idx
        self.ptrs = (_chk(f, "f", F32), _chk(xyz, "xyz", F32), _chk(new_xyz, "new_xyz", F32),
                     _chk(xyz_batch_cnt, "xyz_batch_cnt", I32), _chk(new_xyz_batch_cnt, "new_xyz_batch_cnt", I32),
                     _chk(idx, "idx", I32))


def stack_sa_moments(geo, w1x):
    """-> (2, C1) float64 [sum y1, sum y1^2] over all slots."""
    sums = torch.empty((2, geo.c1), dtype=F64, device=geo.device)
    scratch = _scratch(geo.m, geo.c1, geo.c1, geo.ns, geo.device)
    _call("pda_stack_sa_moments", geo.first, *geo.ptrs, _chk(w1x, "w1x", F32), scratch.data_ptr(), sums.data_ptr(), geo.b, geo.n,
          geo.m, geo.c1, geo.ns)
    return sums


def stack_sa_fwd(geo, w1x, w2, s1, t1, gamma2):
    """-> u (M, C2) the selected extreme of y2, arg (M, C2) uint8 its first slot, (2, C2) float64 [sum y2, sum y2^2]."""
    c2 = w2.shape[0]
    if w1x.shape != (geo.c1, 3) or w2.shape != (c2, geo.c1) or s1.numel() != geo.c1 or t1.numel() != geo.c1 or gamma2.numel() != c2:
        raise ValueError("stack_sa_fwd: shapes disagree")
    u = torch.empty((geo.m, c2), dtype=F32, device=geo.device)
    arg = torch.empty((geo.m, c2), dtype=U8, device=geo.device)
    sums = torch.empty((2, c2), dtype=F64, device=geo.device)
    scratch = _scratch(geo.m, geo.c1, c2, geo.ns, geo.device)
    _call("pda_stack_sa_fwd", geo.first, *geo.ptrs, _chk(w1x, "w1x", F32), _chk(w2, "w2", F32), _chk(s1, "s1", F32),
          _chk(t1, "t1", F32), _chk(gamma2, "gamma2", F32), u.data_ptr(), arg.data_ptr(), scratch.data_ptr(), sums.data_ptr(),
          geo.b, geo.n, geo.m, geo.c1, c2, geo.ns)
    return u, arg, sums


def stack_sa_apply(u, s2, t2):
    out = torch.empty_like(u)
    _call("pda_stack_sa_apply", u, _chk(u, "u", F32), _chk(s2, "s2", F32), _chk(t2, "t2", F32), out.data_ptr(), u.shape[0],
          u.shape[1])
    return out


def stack_sa_bwd1(geo, w1x, w2, s1, t1, arg, g, s2, a2, b2):
    """-> e1 (M, ns, C1), dW2 (C2, C1), sum e1 (C1), sum e1 y1 (C1), the sums float64."""
    c1, c2 = geo.c1, w2.shape[0]
    e1 = torch.empty((geo.m, geo.ns, c1), dtype=F32, device=geo.device)
    sums = torch.empty((c1 * c2 + 2 * c1,), dtype=F64, device=geo.device)
    scratch = _scratch(geo.m, c1, c2, geo.ns, geo.device)
    _call("pda_stack_sa_bwd1", geo.first, *geo.ptrs, _chk(w1x, "w1x", F32), _chk(w2, "w2", F32), _chk(s1, "s1", F32),
          _chk(t1, "t1", F32), _chk(arg, "arg", U8), _chk(g, "g", F32), _chk(s2, "s2", F32), _chk(a2, "a2", F32),
          _chk(b2, "b2", F32), e1.data_ptr(), scratch.data_ptr(), sums.data_ptr(), geo.b, geo.n, geo.m, c1, c2, geo.ns)
    return e1, sums[:c1 * c2].view(c1, c2).t(), sums[c1 * c2:c1 * c2 + c1], sums[c1 * c2 + c1:]


def stack_sa_bwd2(geo, w1x, e1, s1, a1, b1):
    """-> dF (N, C1) float32 (float atomics), dW1x (C1, 3) float64."""
    grad_f = torch.zeros((geo.n, geo.c1), dtype=F32, device=geo.device)
    sums = torch.empty((3, geo.c1), dtype=F64, device=geo.device)
    scratch = _scratch(geo.m, geo.c1, geo.c1, geo.ns, geo.device)
    _call("pda_stack_sa_bwd2", geo.first, *geo.ptrs, _chk(w1x, "w1x", F32), _chk(e1, "e1", F32), _chk(s1, "s1", F32),
          _chk(a1, "a1", F32), _chk(b1, "b1", F32), grad_f.data_ptr(), scratch.data_ptr(), sums.data_ptr(), geo.b, geo.n, geo.m,
          geo.c1, geo.ns)
    return grad_f, sums.t()


class _FusedStackSA(torch.autograd.Function):
    """max over the slots of relu(bn2(W2 relu(bn1(F[g] + W1x rel)))); the BatchNorm buffers are updated as nn.BatchNorm2d does."""

    @staticmethod
    def forward(ctx, f, idx, xyz, new_xyz, xyz_batch_cnt, new_xyz_batch_cnt, w1x, w2, gamma1, beta1, gamma2, beta2, bn1, bn2):
        f = f.contiguous()
        geo = _Geometry(f, xyz, new_xyz, xyz_batch_cnt, new_xyz_batch_cnt, idx)
        n_slots = max(geo.m * geo.ns, 1)
        w1x_c = w1x.detach().contiguous()
        w2_c = w2.detach().reshape(w2.shape[0], geo.c1).contiguous()
        sums1 = stack_sa_moments(geo, w1x_c) if (bn1.training or bn1.running_mean is None) else None
        mean1, var1, batch1 = _statistics(bn1, sums1, n_slots, bn1.training)
        s1, t1, istd1 = bn_scale_shift(gamma1.detach(), beta1.detach(), mean1, var1, bn1.eps)
        s1f, t1f = s1.float(), t1.float()
        u, arg, sums2 = stack_sa_fwd(geo, w1x_c, w2_c, s1f, t1f, gamma2.detach().contiguous())
        mean2, var2, batch2 = _statistics(bn2, sums2, n_slots, bn2.training)
        s2, t2, istd2 = bn_scale_shift(gamma2.detach(), beta2.detach(), mean2, var2, bn2.eps)
        s2f = s2.float()
        out = stack_sa_apply(u, s2f, t2.float())
        ctx.save_for_backward(f, idx, xyz, new_xyz, xyz_batch_cnt, new_xyz_batch_cnt, w1x_c, w2_c, s1f, t1f, s2f, u, arg, out,
                              s1, mean1, istd1, s2, mean2, istd2)
        ctx.misc = (n_slots, batch1, batch2, w1x.shape, w2.shape, w1x.dtype)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (f, idx, xyz, new_xyz, xyz_batch_cnt, new_xyz_batch_cnt, w1x, w2, s1f, t1f, s2f, u, arg, out, s1, mean1, istd1, s2, mean2,
         istd2) = ctx.saved_tensors
        n_slots, batch1, batch2, w1x_shape, w2_shape, dtype = ctx.misc
        geo = _Geometry(f, xyz, new_xyz, xyz_batch_cnt, new_xyz_batch_cnt, idx)
        g = (grad_out * (out > 0)).contiguous()
        gd = g.double()
        dgamma2, dbeta2, a2, b2 = bn_backward_constants(gd.sum(dim=0), (gd * u.double()).sum(dim=0), s2, mean2, istd2, n_slots, batch2)
        e1, dw2, sum_e, sum_ey = stack_sa_bwd1(geo, w1x, w2, s1f, t1f, arg, g, s2f, a2.float(), b2.float())
        dgamma1, dbeta1, a1, b1 = bn_backward_constants(sum_e, sum_ey, s1, mean1, istd1, n_slots, batch1)
        grad_f, dw1x = stack_sa_bwd2(geo, w1x, e1, s1f, a1.float(), b1.float())
        return (grad_f, None, None, None, None, None, dw1x.to(dtype).reshape(w1x_shape), dw2.to(dtype).reshape(w2_shape),
                dgamma1.to(dtype), dbeta1.to(dtype), dgamma2.to(dtype), dbeta2.to(dtype), None, None)


def fused_stack_sa(features, idx, xyz, new_xyz, xyz_batch_cnt, new_xyz_batch_cnt, conv1, bn1, conv2, bn2):
    """One scale: features (N, C_in), idx (M, nsample) the stacked ball query's raw output (LOCAL rows, first slot -1 for an
    empty ball), the two Conv2d / BatchNorm2d pairs -> (M, C2)."""
    w1 = conv1.weight[:, :, 0, 0]
    f = features @ w1[:, 3:].t()
    return _FusedStackSA.apply(f, idx, xyz, new_xyz, xyz_batch_cnt, new_xyz_batch_cnt, w1[:, :3], conv2.weight, bn1.weight,
                               bn1.bias, bn2.weight, bn2.bias, bn1, bn2)


class StackSAModuleMSG(nn.Module):
    def __init__(self, *, radii, nsamples, mlps, use_xyz=True, pool_method='max_pool'):
        super().__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for i in range(len(radii)):
            self.groupers.append(pointnet2_utils.QueryAndGroup(radii[i], nsamples[i], use_xyz=use_xyz))
            mlp_spec = list(mlps[i])                    # a copy: the caller's list (the model config) stays as it is
            if use_xyz:
                mlp_spec[0] += 3
            shared_mlps = []
            for k in range(len(mlp_spec) - 1):
                shared_mlps.extend([nn.Conv2d(mlp_spec[k], mlp_spec[k + 1], kernel_size=1, bias=False),
                                    nn.BatchNorm2d(mlp_spec[k + 1]), nn.ReLU()])
            self.mlps.append(nn.Sequential(*shared_mlps))
        if pool_method not in ('max_pool', 'avg_pool'):
            raise NotImplementedError(pool_method)
        self.pool_method = pool_method
        self.use_xyz = use_xyz
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def is_fused(self, k):
        """Whether scale k takes the fused kernels now (given features)."""
        mlp = self.mlps[k]
        return (sa_path() == "fused" and self.pool_method == 'max_pool' and self.use_xyz and len(mlp) == 6
                and mlp[0].out_channels in FUSED_CHANNELS and mlp[3].out_channels in FUSED_CHANNELS
                and 1 <= self.groupers[k].nsample <= FUSED_MAX_NSAMPLE)

    def _scale_fused(self, k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features):
        g = self.groupers[k]
        M = new_xyz.shape[0]
        idx = torch.zeros((M, g.nsample), dtype=torch.int32, device=xyz.device)
        pointnet2.ball_query_wrapper(xyz_batch_cnt.shape[0], M, g.radius, g.nsample, new_xyz, new_xyz_batch_cnt, xyz,
                                     xyz_batch_cnt, idx)
        conv1, bn1, _, conv2, bn2, _ = self.mlps[k]
        return fused_stack_sa(features, idx, xyz, new_xyz, xyz_batch_cnt, new_xyz_batch_cnt, conv1, bn1, conv2, bn2)

    def _scale_composed(self, k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features):
        """pointnet2_modules.py:91-107"""
        new_features, _ = self.groupers[k](xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features)   # (M, C, nsample)
        new_features = new_features.permute(1, 0, 2).unsqueeze(dim=0)                                  # (1, C, M, nsample)
        new_features = self.mlps[k](new_features)
        if self.pool_method == 'max_pool':
            new_features = F.max_pool2d(new_features, kernel_size=[1, new_features.size(3)]).squeeze(dim=-1)
        else:
            new_features = F.avg_pool2d(new_features, kernel_size=[1, new_features.size(3)]).squeeze(dim=-1)
        return new_features.squeeze(dim=0).permute(1, 0)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None, empty_voxel_set_zeros=True):
        """xyz (N1 + N2 ..., 3), new_xyz (M1 + M2 ..., 3), the int32 counts per scene, features (N, C_in) ->
        new_xyz, new_features (M, sum_k mlps[k][-1])."""
        xyz, new_xyz = xyz.contiguous(), new_xyz.contiguous()
        new_features_list = []
        for k in range(len(self.groupers)):
            if features is not None and self.is_fused(k):
                new_features = self._scale_fused(k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features.contiguous())
            else:
                sa_path()                               # a bad value raises on either path
                new_features = self._scale_composed(k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features)
            new_features_list.append(new_features)
        return new_xyz, torch.cat(new_features_list, dim=1)


class VectorPoolAggregationModuleMSG(nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("VectorPoolAggregationModuleMSG (PV-RCNN++) is not part of this project")


def build_local_aggregation_module(input_channels, config):
    """-> (layer, its output width).  config.MLPS is read, not modified."""
    name = config.get('NAME', 'StackSAModuleMSG')
    if name == 'StackSAModuleMSG':
        mlps = [[input_channels] + list(m) for m in config['MLPS']]
        layer = StackSAModuleMSG(radii=config['POOL_RADIUS'], nsamples=config['NSAMPLE'], mlps=mlps, use_xyz=True,
                                 pool_method='max_pool')
        return layer, sum(x[-1] for x in mlps)
    if name == 'VectorPoolAggregationModuleMSG':
        return VectorPoolAggregationModuleMSG(input_channels=input_channels, config=config), config['MSG_POST_MLPS'][-1]
    raise NotImplementedError(name)
