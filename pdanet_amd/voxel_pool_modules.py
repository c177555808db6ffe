"""NeighborVoxelSAModuleMSG (pcdet/ops/pointnet2/pointnet2_stack/voxel_pool_modules.py): the RoI-grid pooling layer of
Voxel R-CNN, under the reference's constructor, module names (groupers, mlps_in, mlps_pos, mlps_out) and state-dict keys.

Two paths compute one scale after mlps_in:
  fused     csrc/voxel_pool.hip: the voxel query's idx goes straight into three entries (moments, forward, backward); the
            (1, C, M, nsample) tensors of the reference -- grouped features, position conv, its BatchNorm, the sum, the
            ReLU -- are never made.  max_pool with C = 32 or 64.
  composed  the reference's sequence over VoxelQueryAndGrouping and torch modules.  Taken for avg_pool and any other C, and
            for every layer with PDA_VOXEL_POOL=composed (the benchmark's baseline, tools/voxel_pool_bench.py).

BatchNorm2d(W rel) in the fused path.  y = W x is linear in the 3-vector x = rel, so over the n = M * nsample slots
    mean_c = w_c . mu,   var_c = w_c^T Sigma w_c,   mu = S1 / n,   Sigma = S2 / n - mu mu^T
from S1 = sum x (3 numbers) and S2 = sum x x^T (6 numbers), which pda_voxel_pool_moments leaves in float64.  The kernel
gets scale = gamma / sigma and shift = beta - mean * scale (sigma = sqrt(var + eps)); in eval mode they come from the running
statistics.  The backward is closed form too: with g the incoming gradient where out > 0 and x* the winner's rel,
    dbeta_c = sum g,   dgamma_c = (sum g (w_c . x*) - mean_c dbeta_c) / sigma_c
    dW_c = (gamma_c / sigma_c) (sum g x*^T - dbeta_c / n S1^T - dgamma_c / n (w_c^T S2 - mean_c S1^T) / sigma_c)
finished here in float64 from the kernel's per-channel sums (`moment_finish`, `moment_backward`: plain torch, any device)."""
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import pointnet2_stack_cuda as pointnet2
from . import pointnet2_stack_utils as voxel_query_utils
from ._lib import load as _load
from .config import fused_or_composed
from .pointnet2_batch_cuda import F32, I32, _call, _chk

# 'fused' (default) or 'composed', read when a layer runs
ENV = "PDA_VOXEL_POOL"
pool_path = partial(fused_or_composed, ENV)
FUSED_CHANNELS = (32, 64)


def _sym(s2):
    """[xx, xy, xz, yy, yz, zz] -> the symmetric (3, 3) matrix."""
    return torch.stack([s2[0], s2[1], s2[2], s2[1], s2[3], s2[4], s2[2], s2[4], s2[5]]).view(3, 3)


def moment_finish(sums, n, w):
    """sums (9) float64 [S1, S2 upper triangle], n slots, w (C, 3) -> (mean, var) (C) float64, var biased."""
    w = w.double()
    mu = sums[:3] / n
    sigma = _sym(sums[3:]) / n - torch.outer(mu, mu)
    return w @ mu, ((w @ sigma) * w).sum(dim=1).clamp(min=0)


def moment_backward(win, sums, n, w, gamma, mean, var, eps, batch_stats):
    """win (5, C) float64 [sum g, sum g (w . x*), sum g x*], sums / n as in moment_finish, mean / var the statistics the
    forward normalised with -> (dW (C, 3), dgamma, dbeta) float64.  batch_stats False (eval mode): mean and var are
    constants and the two correction terms of dW drop out."""
    w, gamma = w.double(), gamma.double()
    sigma = torch.sqrt(var + eps)
    dbeta = win[0]
    dgamma = (win[1] - mean * dbeta) / sigma
    dw = win[2:5].t()
    if batch_stats:
        s1 = sums[:3]
        yhat_x = (w @ _sym(sums[3:]) - mean[:, None] * s1[None, :]) / sigma[:, None]
        dw = dw - dbeta[:, None] / n * s1[None, :] - dgamma[:, None] / n * yhat_x
    return (gamma / sigma)[:, None] * dw, dgamma, dbeta


def _scratch(m, c, nsample, device):
    need = _load().pda_voxel_pool_scratch_doubles(m, c, nsample)
    if need < 0:
        raise ValueError("voxel pool: m=%d c=%d nsample=%d is outside the fused kernels (c 32 or 64, nsample 1..255)" % (m, c, nsample))
    return torch.empty((max(int(need), 1),), dtype=torch.float64, device=device)


def voxel_pool_moments(idx, xyz, new_xyz):
    """idx (M, ns) int32 as the voxel query leaves it, xyz (N, 3), new_xyz (M, 3) -> (9) float64 sums of rel."""
    m, ns = idx.shape
    sums = torch.empty(9, dtype=torch.float64, device=idx.device)
    scratch = _scratch(m, FUSED_CHANNELS[0], ns, idx.device)
    _call("pda_voxel_pool_moments", idx, _chk(idx, "idx", I32), _chk(xyz, "xyz", F32), _chk(new_xyz, "new_xyz", F32),
          scratch.data_ptr(), sums.data_ptr(), xyz.shape[0], m, ns)
    return sums


def voxel_pool_fwd(features_in, idx, xyz, new_xyz, w, scale, shift):
    """-> out (M, C) float32, arg (M, C) uint8 (csrc/voxel_pool.hip states the value and the tie rule)."""
    m, ns = idx.shape
    n, c = features_in.shape
    if xyz.shape[0] != n or new_xyz.shape[0] != m or w.numel() != c * 3 or scale.numel() != c or shift.numel() != c:
        raise ValueError("voxel_pool_fwd: shapes disagree")
    out = torch.empty((m, c), dtype=F32, device=idx.device)
    arg = torch.empty((m, c), dtype=torch.uint8, device=idx.device)
    _call("pda_voxel_pool_fwd", idx, _chk(features_in, "features_in", F32), _chk(idx, "idx", I32), _chk(xyz, "xyz", F32),
          _chk(new_xyz, "new_xyz", F32), _chk(w, "w", F32), _chk(scale, "scale", F32), _chk(shift, "shift", F32),
          out.data_ptr(), arg.data_ptr(), n, m, c, ns)
    return out, arg


def voxel_pool_bwd(grad_out, out, arg, idx, xyz, new_xyz, w, n):
    """-> grad_features_in (n, C) float32 (float atomics), winner sums (5, C) float64."""
    m, ns = idx.shape
    c = out.shape[1]
    grad_feat = torch.zeros((n, c), dtype=F32, device=idx.device)
    win = torch.empty((5, c), dtype=torch.float64, device=idx.device)
    scratch = _scratch(m, c, ns, idx.device)
    _call("pda_voxel_pool_bwd", idx, _chk(grad_out, "grad_out", F32), _chk(out, "out", F32), _chk(arg, "arg", torch.uint8),
          _chk(idx, "idx", I32), _chk(xyz, "xyz", F32), _chk(new_xyz, "new_xyz", F32), _chk(w, "w", F32),
          grad_feat.data_ptr(), scratch.data_ptr(), win.data_ptr(), n, m, c, ns)
    return grad_feat, win


class _FusedVoxelPool(torch.autograd.Function):
    """relu(f + BatchNorm2d(W rel)) max-pooled over the slots; BatchNorm's buffers are updated as nn.BatchNorm2d does."""

    @staticmethod
    def forward(ctx, features_in, idx, xyz, new_xyz, weight, gamma, beta, bn, training):
        m, ns = idx.shape
        n_slots = m * ns
        w = weight.detach().reshape(weight.shape[0], 3).contiguous()
        batch_stats = training or bn.running_mean is None
        sums = None
        if batch_stats:
            sums = voxel_pool_moments(idx, xyz, new_xyz)
            mean, var = moment_finish(sums, n_slots, w)
            if training and bn.running_mean is not None:
                bn.num_batches_tracked += 1
                mom = bn.momentum if bn.momentum is not None else 1.0 / bn.num_batches_tracked.double()
                unbiased = var * (n_slots / max(n_slots - 1, 1))
                bn.running_mean.mul_(1 - mom).add_((mom * mean).to(bn.running_mean.dtype))
                bn.running_var.mul_(1 - mom).add_((mom * unbiased).to(bn.running_var.dtype))
        else:
            mean, var = bn.running_mean.double(), bn.running_var.double()
        scale = gamma.detach().double() / torch.sqrt(var + bn.eps)
        shift = beta.detach().double() - mean * scale
        out, arg = voxel_pool_fwd(features_in.contiguous(), idx, xyz, new_xyz, w, scale.float(), shift.float())
        ctx.save_for_backward(out, arg, idx, xyz, new_xyz, w, gamma.detach(), mean, var, sums)
        ctx.misc = (features_in.shape[0], n_slots, bn.eps, batch_stats, weight.shape)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, grad_out, _grad_arg=None):
        out, arg, idx, xyz, new_xyz, w, gamma, mean, var, sums = ctx.saved_tensors
        n, n_slots, eps, batch_stats, w_shape = ctx.misc
        grad_feat, win = voxel_pool_bwd(grad_out.contiguous(), out, arg, idx, xyz, new_xyz, w, n)
        dw, dgamma, dbeta = moment_backward(win, sums, n_slots, w, gamma, mean, var, eps, batch_stats)
        return (grad_feat, None, None, None, dw.to(w.dtype).view(w_shape), dgamma.to(gamma.dtype), dbeta.to(gamma.dtype),
                None, None)


def fused_voxel_pool(features_in, idx, xyz, new_xyz, conv, bn, training):
    """One scale after mlps_in: features_in (N, C), idx (M, nsample) the voxel query's raw output (GLOBAL rows, first slot
    -1 for an empty ball), conv / bn the two modules of mlps_pos -> (M, C)."""
    return _FusedVoxelPool.apply(features_in, idx, xyz, new_xyz, conv.weight, bn.weight, bn.bias, bn, training)[0]


class NeighborVoxelSAModuleMSG(nn.Module):
    def __init__(self, *, query_ranges, radii, nsamples, mlps, use_xyz=True, pool_method='max_pool'):
        super().__init__()
        assert len(query_ranges) == len(nsamples) == len(mlps)
        self.groupers = nn.ModuleList()
        self.mlps_in = nn.ModuleList()
        self.mlps_pos = nn.ModuleList()
        self.mlps_out = nn.ModuleList()
        for i in range(len(query_ranges)):
            self.groupers.append(voxel_query_utils.VoxelQueryAndGrouping(query_ranges[i], radii[i], nsamples[i]))
            spec = mlps[i]
            self.mlps_in.append(nn.Sequential(nn.Conv1d(spec[0], spec[1], kernel_size=1, bias=False), nn.BatchNorm1d(spec[1])))
            self.mlps_pos.append(nn.Sequential(nn.Conv2d(3, spec[1], kernel_size=1, bias=False), nn.BatchNorm2d(spec[1])))
            self.mlps_out.append(nn.Sequential(nn.Conv1d(spec[1], spec[2], kernel_size=1, bias=False), nn.BatchNorm1d(spec[2]),
                                               nn.ReLU()))
        self.relu = nn.ReLU()
        if pool_method not in ('max_pool', 'avg_pool'):
            raise NotImplementedError(pool_method)
        self.pool_method = pool_method
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def is_fused(self, k):
        """Whether scale k takes the fused kernels now."""
        return pool_path() == "fused" and self.pool_method == 'max_pool' and self.mlps_pos[k][0].out_channels in FUSED_CHANNELS

    def _pool_fused(self, k, new_coords, xyz, new_xyz, features_in, voxel2point_indices):
        g = self.groupers[k]
        M = new_coords.shape[0]
        _, Z, Y, X = voxel2point_indices.shape
        idx = torch.zeros((M, g.nsample), dtype=torch.int32, device=xyz.device)
        z_range, y_range, x_range = g.max_range
        pointnet2.voxel_query_wrapper(M, Z, Y, X, g.nsample, g.radius, z_range, y_range, x_range, new_xyz, xyz, new_coords,
                                      voxel2point_indices, idx)
        conv, bn = self.mlps_pos[k]
        return fused_voxel_pool(features_in, idx, xyz, new_xyz, conv, bn, bn.training).t().unsqueeze(0)

    def _pool_composed(self, k, new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features_in, voxel2point_indices):
        """voxel_pool_modules.py:96-121; the masks are applied out of place."""
        grouped_features, grouped_xyz, empty = self.groupers[k](new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt,
                                                                features_in, voxel2point_indices)
        empty = empty[:, None, None]
        grouped_features = grouped_features.masked_fill(empty, 0).permute(1, 0, 2).unsqueeze(dim=0)
        grouped_xyz = (grouped_xyz - new_xyz.unsqueeze(-1)).masked_fill(empty, 0).permute(1, 0, 2).unsqueeze(0)
        new_features = self.relu(grouped_features + self.mlps_pos[k](grouped_xyz))
        if self.pool_method == 'max_pool':
            return F.max_pool2d(new_features, kernel_size=[1, new_features.size(3)]).squeeze(dim=-1)
        return F.avg_pool2d(new_features, kernel_size=[1, new_features.size(3)]).squeeze(dim=-1)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices):
        """xyz (N1 + N2 ..., 3), new_xyz (M1 + M2 ..., 3), new_coords (M, 4) [batch, x, y, z] int32, features (N, C_in),
        voxel2point_indices (B, Z, Y, X) -> (M, sum_k mlps[k][-1])."""
        new_coords = new_coords[:, [0, 3, 2, 1]].contiguous()          # [batch_idx, z, y, x]
        new_features_list = []
        for k in range(len(self.groupers)):
            features_in = self.mlps_in[k](features.permute(1, 0).unsqueeze(0))
            features_in = features_in.permute(0, 2, 1).contiguous().view(-1, features_in.shape[1])
            if self.is_fused(k):
                new_features = self._pool_fused(k, new_coords, xyz, new_xyz, features_in, voxel2point_indices)
            else:
                new_features = self._pool_composed(k, new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features_in,
                                                   voxel2point_indices)
            new_features = self.mlps_out[k](new_features)               # (1, C, M)
            new_features_list.append(new_features.squeeze(dim=0).permute(1, 0))
        return torch.cat(new_features_list, dim=1)
