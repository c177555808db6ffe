#!/usr/bin/env python
"""Generates tests/golden/pointrcnn.npz and tests/golden/pointrcnn_state_dict.json from the REFERENCE's own
pointnet2_batch/pointnet2_modules.py, pointnet2_backbone.py, point_head_box.py, box_coder_utils.py, roipoint_pool3d_utils.py
and pointrcnn_head.py, imported from where they lie and run on the CPU in float32 and again in float64.

    python tests/golden/make_pointrcnn_golden.py <checkout of the reference>

Stubs: `pointnet2_batch_cuda` over the repository's C oracle (ball query, farthest-point sampling, three_nn; the grouping,
gathering and interpolation entries are numpy gathers in the dtype of the run), `roipoint_pool3d_cuda` over
roi_pool_restatement.py, `points_in_boxes_gpu` over stack_sa_restatement.py, the NMS and the RoI sampling by what
make_roi_targets_golden.py uses (its run_targets, which records the reference's draws).  Nothing of the reference is copied;
what is committed is data.  The float64 run (reference_loader.precision) points the reference's float allocator at the double
constructor and lets .float() return a double, so that the reference's own allocations and casts follow the run's precision;
every input of it is a float32 value.

pointrcnn.npz -- every float output as <key> (float32 run) and <key>_f64:
  sa_*   one PointnetSAModuleMSG (npoint 32, two scales) and one PointnetSAModule(npoint=None) on 2 x 128 points: train and
         eval output, the sampled centres, the running statistics after the train step.
  fp_*   one PointnetFPModule, called as PointNet2MSG calls it: train and eval output.
  bb_*   PointNet2MSG on 2 x 256 points (NPOINTS [64, 16, 8, 4], the yaml's NSAMPLE): point_features in train and eval mode.
  ph_*   PointHeadBox (3 classes, mean sizes): labels, box labels, both losses, the parameter gradients, eval's decoded boxes;
         PointResidualCoder's codes and decoded boxes with and without mean sizes.
  rh_*   PointRCNNHead (S = 16, C = 8, SA NPOINTS [8, 4, -1]): the pooled input, rcnn_cls / rcnn_reg in train mode (on the
         RoIs the recorded draws sample) and eval mode (on the given RoIs), the train-mode output of each SA level, the three
         losses, the parameter gradients, eval's decoded boxes.

Coordinates lie on the 1/8 lattice.  The generator fails (a part then tries its next seed) when
 (a) in ph_* or rh_*, whose gradients are stored, a ReLU input of the float64 train run lies within 1e-3 of its tensor's largest
     magnitude of zero, or the winner of a max over nsample leads the next distinct value by less than WIN_MARGIN = 2e-5 of the
     tensor's largest magnitude (the margin of make_pv_rcnn_golden.py, condition (a)).  Random parameters cannot meet the first
     part, so those two modules' parameters are CONSTRUCTED as there: every BatchNorm has |bias| well above |weight| times the
     spread of a normalised value, biases of both signs (every fifth channel is dead behind its ReLU); the head's two
     Conv2d + ReLU layers without BatchNorm have small weights under biases of both signs.  Behind such ReLUs an activation is a
     large constant plus a small signal; both modules' contractions that a BatchNorm follows are therefore centred on the train
     batch (`centre`), so that a BatchNorm's input has zero mean and the fixture measures the head, not how a variance is summed;
 (b) a ball-query distance lies within 1e-3 of its radius;
 (d) in rh_*, whose sampling runs on canonical coordinates that the reference and the device round differently, a round of a
     farthest-point sampling is decided by less than 1e-4 of the winner's squared distance (points at the winner's own
     coordinates apart: a RoI with fewer than S points repeats them); the scene's coordinates are in general position for that;
 (e) in ph_* or rh_*, a loss or a parameter gradient (sums over the batch) of the float32 run lies closer to the float64 run than float32 can promise: 0 < e <
     2^-24 of the tensor's largest magnitude, which for a scalar or a short vector happens by luck.  The tests allow the device
     4 e, and such an e is no measure of the reference's rounding;
 (c) a box-membership limit (half extents of the ground-truth boxes, their enlarged twins and the RoIs) lies within 1e-4 of a
     point's local coordinate.

pointrcnn_state_dict.json: keys and shapes, in order, of the reference's PointNet2MSG, PointHeadBox and PointRCNNHead for
kitti_models/pointrcnn.yaml (3 classes, 4 point features), of the whole PointRCNN in the reference's module order, and the
config used."""
import copy
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from reference_loader import load, model_yaml, precision, randomise, reference_root, shapes, state, write_state_dict  # noqa: E402
import make_roi_targets_golden as rt  # noqa: E402  (the scenes and run_targets, which records the reference's draws)
import oracle  # noqa: E402
import roi_pool_restatement as rp  # noqa: E402
from pdanet_amd.config import to_attr  # noqa: E402

F32, I32, F64 = np.float32, np.int32, np.float64
WIN_MARGIN = 2e-5
t = torch.from_numpy
QUERIES = []                     # (radius, new_xyz (B, M, 3), xyz (B, N, 3)) of every ball query made, for condition (b)
SAMPLINGS = []                   # (xyz (B, N, 3), npoint) of every farthest-point sampling made, for condition (d)


def _c32(x):
    return np.ascontiguousarray(x.detach().numpy(), dtype=F32)


class Stub(types.ModuleType):
    """pointnet2_batch_cuda on CPU tensors of either precision: the queries run in float32 (every coordinate is a float32
    value), the gathers in the tensors' own type."""

    def __init__(self):
        super().__init__("pointnet2_batch_cuda")

    @staticmethod
    def ball_query_wrapper(B, N, M, radius, nsample, new_xyz, xyz, idx):
        QUERIES.append((float(radius), new_xyz.detach().numpy().astype(F64), xyz.detach().numpy().astype(F64)))
        return oracle.ball_query_wrapper(B, N, M, radius, nsample, _c32(new_xyz), _c32(xyz), idx.numpy())

    @staticmethod
    def farthest_point_sampling_wrapper(B, N, npoint, xyz, temp, idx):
        SAMPLINGS.append((xyz.detach().numpy().astype(F64), int(npoint)))
        return oracle.farthest_point_sampling_wrapper(B, N, npoint, _c32(xyz), np.full((B, N), 1e10, F32), idx.numpy())

    @staticmethod
    def group_points_wrapper(B, C, N, npoints, nsample, points, idx, out):
        p, i = points.detach().numpy(), idx.numpy().astype(np.int64)
        for b in range(B):
            out.numpy()[b] = p[b][:, i[b]]
        return 1

    @staticmethod
    def group_points_grad_wrapper(B, C, N, npoints, nsample, grad_out, idx, grad_points):
        g, i, acc = grad_out.detach().numpy(), idx.numpy().astype(np.int64), grad_points.numpy()
        for b in range(B):                                 # one add after the other in (centre, slot) order, in the run's type
            np.add.at(acc[b].T, i[b].reshape(-1), g[b].reshape(C, -1).T)
        return 1

    @staticmethod
    def gather_points_wrapper(B, C, N, npoints, points, idx, out):
        p, i = points.detach().numpy(), idx.numpy().astype(np.int64)
        for b in range(B):
            out.numpy()[b] = p[b][:, i[b]]
        return 1

    @staticmethod
    def gather_points_grad_wrapper(B, C, N, npoints, grad_out, idx, grad_points):
        g, i, acc = grad_out.detach().numpy(), idx.numpy().astype(np.int64), grad_points.numpy()
        for b in range(B):
            np.add.at(acc[b].T, i[b], g[b].T)
        return 1

    @staticmethod
    def three_nn_wrapper(B, N, M, unknown, known, dist2, idx):
        d = np.zeros((B, N, 3), F32)
        oracle.three_nn_wrapper(B, N, M, _c32(unknown), _c32(known), d, idx.numpy())
        dist2.numpy()[...] = d                              # lattice coordinates: the squared distances are exact in float32
        return 1

    @staticmethod
    def three_interpolate_wrapper(B, C, M, N, points, idx, weight, out):
        p, i, w = points.detach().numpy(), idx.numpy().astype(np.int64), weight.detach().numpy()
        for b in range(B):
            g = p[b][:, i[b]]                              # (C, N, 3)
            out.numpy()[b] = (g[:, :, 0] * w[b][None, :, 0] + g[:, :, 1] * w[b][None, :, 1]) + g[:, :, 2] * w[b][None, :, 2]
        return 1

    @staticmethod
    def three_interpolate_grad_wrapper(B, C, N, M, grad_out, idx, weight, grad_points):
        g, i, w, acc = grad_out.detach().numpy(), idx.numpy().astype(np.int64), weight.detach().numpy(), grad_points.numpy()
        for b in range(B):
            for k in range(3):
                np.add.at(acc[b].T, i[b][:, k], (g[b] * w[b][None, :, k]).T)
        return 1


def _roipoint_forward(xyz, boxes3d, pts_feature, pooled_features, pooled_empty_flag):
    return rp.roipoint_pool3d_forward(xyz.numpy(), boxes3d.numpy(), pts_feature.numpy(), pooled_features.numpy(),
                                      pooled_empty_flag.numpy())


def load_reference(root):
    """-> (pointnet2_modules, pointnet2_backbone, box_coder_utils, point_head_box, pointrcnn_head) of the reference, beside what
    make_roi_targets_golden loads as pcdet_ref.*"""
    rt.load_reference(root)
    batch = "ops.pointnet2.pointnet2_batch."
    # pointnet2_backbone.py imports the stack package for PointNet2Backbone, which nothing here builds
    stubs = {batch + "pointnet2_batch_cuda": Stub(), batch + "semantic_view": {},
             "ops.pointnet2.pointnet2_stack": {"pointnet2_modules": types.ModuleType("pointnet2_modules"),
                                               "pointnet2_utils": types.ModuleType("pointnet2_utils")},
             "ops.roipoint_pool3d.roipoint_pool3d_cuda": {"forward": _roipoint_forward}}
    load(root, "pcdet_ref", [batch + "pointnet2_utils", batch + "PointFormer", "ops.roipoint_pool3d.roipoint_pool3d_utils",
                             "models.dense_heads.point_head_template"], stubs=stubs)
    pm, bb, ph, rh = load(root, "pcdet_ref", [batch + "pointnet2_modules", "models.backbones_3d.pointnet2_backbone",
                                              "models.dense_heads.point_head_box", "models.roi_heads.pointrcnn_head"])
    return pm, bb, rt.CODER, ph, rh


RUNS = ((torch.float32, ""), (torch.float64, "_f64"))


def cast(x, dtype):
    """a numpy array as a tensor of the run: floats in `dtype`, the rest as they are"""
    x = t(np.array(x))
    return x.to(dtype) if x.is_floating_point() else x


def check_radii(what):
    """condition (b) over the queries recorded since the last call"""
    worst = np.inf
    for radius, new_xyz, xyz in QUERIES:
        d = np.sqrt(((new_xyz[:, :, None, :] - xyz[:, None, :, :]) ** 2).sum(-1))
        worst = min(worst, float(np.abs(d - radius).min()))
    print("%s: %d ball queries, the nearest distance to a radius is %.4f" % (what, len(QUERIES), worst))
    del QUERIES[:]
    return worst > 1e-3


def check_samplings(what):
    """condition (d) over the samplings recorded since the last call: in every round the farthest point leads the farthest
    point at OTHER coordinates (a repeated point ties with its twin harmlessly) by more than 1e-4 of its distance"""
    worst = np.inf
    for xyz, npoint in SAMPLINGS:
        for pts in xyz:
            temp, old = np.full(len(pts), 1e10), 0
            for _ in range(1, min(npoint, len(pts))):
                temp = np.minimum(temp, ((pts - pts[old]) ** 2).sum(-1))
                old = int(np.argmax(temp))
                if temp[old] == 0:
                    break                                  # only repeats of sampled points are left
                other = temp[(pts != pts[old]).any(-1)]
                if len(other):
                    worst = min(worst, float((temp[old] - other.max()) / temp[old]))
    print("%s: %d samplings, the closest decision leads by %.2e of its squared distance" % (what, len(SAMPLINGS), worst))
    del SAMPLINGS[:]
    return worst > 1e-4


def box_margin(points, boxes):
    """condition (c) over the points (N, 3) and boxes (T, 7) of one scene, in float64: a point is inside when the largest of its
    three |local coordinate| - half extent is negative; the least magnitude of that largest, i.e. how far the nearest
    membership decision is from turning"""
    p, b = points.astype(F64)[None], boxes.astype(F64)[:, None]
    d = p - b[..., 0:3]
    c, s = np.cos(-b[..., 6]), np.sin(-b[..., 6])
    lx, ly = d[..., 0] * c - d[..., 1] * s, d[..., 0] * s + d[..., 1] * c
    over = np.maximum(np.maximum(np.abs(lx) - b[..., 3] / 2, np.abs(ly) - b[..., 4] / 2), np.abs(d[..., 2]) - b[..., 5] / 2)
    return float(np.abs(over).min()) if boxes.size and points.size else np.inf


def lattice(rng, n, lo, hi, step=8):
    return np.stack([rng.integers(lo[k], hi[k], n) for k in range(3)], axis=1).astype(F32) / step


def distinct_lattice(rng, n, lo, hi):
    xyz = np.unique(lattice(rng, 2 * n + 40, lo, hi), axis=0)
    xyz = xyz[rng.permutation(len(xyz))[:n]]
    assert len(xyz) == n
    return xyz


def off_lattice(k):
    """a radius whose square falls between two lattice values k / 64"""
    return float(np.sqrt((k + 0.5) / 64))


class Margins:
    """Condition (a) over one float64 train-mode run: hooks on every ReLU, and on the max over nsample."""

    def __init__(self, module, pool_owner=None):
        self.worst_relu, self.worst_win = np.inf, np.inf
        self.module, self.owner = module, pool_owner

    def __enter__(self):
        self.handles = [m.register_forward_pre_hook(self._relu) for m in self.module.modules() if isinstance(m, nn.ReLU)]
        if self.owner is not None:                             # the module whose `F` the reference's SA forward pools through
            functional, record = torch.nn.functional, self._pool

            class _F:
                def __getattr__(self, name):
                    return getattr(functional, name)

                def max_pool2d(self, x, kernel_size):
                    record(x)
                    return functional.max_pool2d(x, kernel_size=kernel_size)
            self.owner.F = _F()
        return self

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()
        if self.owner is not None:
            self.owner.F = torch.nn.functional

    def _relu(self, mod, args):
        x = args[0].detach()
        if x.numel():
            self.worst_relu = min(self.worst_relu, float(x.abs().min() / x.abs().max()))

    def _pool(self, x):
        x = x.detach()
        top = x.max(dim=-1, keepdim=True)[0]
        gap = torch.where(x < top, top - x, torch.full_like(x, float('inf'))).min(dim=-1)[0]
        self.worst_win = min(self.worst_win, float(gap.min() / x.abs().max()))

    def failed(self):
        if self.worst_relu <= 1e-3:
            return "a ReLU input at %.2e of its tensor's largest magnitude" % self.worst_relu
        if self.worst_win <= WIN_MARGIN:
            return "a pooling winner leads by %.2e of its tensor's largest magnitude" % self.worst_win
        return None


def construct(module, rng):
    """The parameters of condition (a), see the module docstring."""
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    r = lambda *s: torch.rand(*s, generator=g)
    sign = lambda n: torch.randint(0, 2, (n,), generator=g) * 2 - 1
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
                c = m.num_features
                m.weight.copy_((0.05 + 0.05 * r(c)) * sign(c))
                bias = 1.0 + 0.5 * r(c)
                bias[::5] *= -1
                m.bias.copy_(bias)
                m.running_mean.copy_((r(c) - 0.5) * 0.1)
                m.running_var.copy_(1.0 + r(c))
            elif isinstance(m, (nn.Conv1d, nn.Conv2d, nn.Linear)):
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / fan_in ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)


def centre(module, run):
    """Behind bias-dominated ReLUs every activation is a large constant plus a small signal, so the next contraction's output
    would have a mean many times its spread, and a BatchNorm over it would measure the summation order of the variance, not the
    module.  One train-mode pass, layer by layer: each contraction without bias (the ones a BatchNorm follows) gets the
    component of its rows along the batch's mean input removed, so that its output has zero mean on this batch.  Prints the
    largest |mean| / spread of a BatchNorm input before and after."""
    def ratio_hook(log):
        def hook(mod, args):
            x = args[0].detach().transpose(0, 1).reshape(args[0].shape[1], -1).double()
            log.append(float((x.mean(1).abs() / x.std(1).clamp(min=1e-30)).max()))
        return hook

    def centre_hook(mod, args):
        x = args[0].detach()
        x = x.reshape(-1, x.shape[-1]) if isinstance(mod, nn.Linear) else x.transpose(0, 1).reshape(x.shape[1], -1).t()
        m = x.double().mean(0)
        w = mod.weight.detach().double().reshape(mod.weight.shape[0], -1)
        with torch.no_grad():
            mod.weight.copy_((w - (w @ m)[:, None] * m[None, :] / (m @ m)).reshape(mod.weight.shape).to(mod.weight.dtype))

    bns = [m for m in module.modules() if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d))]
    figures = []
    for step in ("before", "centre", "after"):
        log = []
        handles = [m.register_forward_pre_hook(ratio_hook(log)) for m in bns]
        if step == "centre":
            handles += [m.register_forward_pre_hook(centre_hook) for m in module.modules()
                        if isinstance(m, (nn.Conv1d, nn.Conv2d, nn.Linear)) and m.bias is None]
        state_before = copy.deepcopy({k: v for k, v in module.state_dict().items() if 'running' in k or 'num_batches' in k})
        module.train()
        with torch.no_grad():
            run(module)
        module.load_state_dict(state_before, strict=False)           # the pass must not move the running statistics
        for h in handles:
            h.remove()
        figures.append(max(log))
    print("largest |mean| / spread of a BatchNorm input: %.1f before, %.2e after centring" % (figures[0], figures[2]))


def lucky(res, prefix):
    """condition (e): the first loss or parameter gradient whose float32 run lies closer to the float64 run than float32 can promise
    (0 < e < 2^-24 of the tensor's largest magnitude), or None.  Tensors that are zero in exact arithmetic have no e."""
    keys = [k for k in res if k.startswith(prefix) and k + "_f64" in res and ("loss" in k or "grad." in k)]
    largest_grad = max(float(np.abs(res[k + "_f64"]).max()) for k in keys if "grad." in k)
    for k in keys:
        r64 = np.asarray(res[k + "_f64"], F64)
        scale = float(np.abs(r64).max())
        if r64.dtype.kind != 'f' or scale == 0 or ("grad." in k and scale <= 1e-12 * largest_grad):
            continue
        e = float(np.abs(np.asarray(res[k], F64) - r64).max()) / scale
        if 0 < e < 2.0 ** -24:
            return "%s: e = %.2e" % (k, e)
    return None


def grads(module, prefix, out, suffix):
    for k, p in module.named_parameters():
        out[prefix + "grad." + k + suffix] = p.grad.detach().numpy().copy()


# ---- sa_*, fp_* -------------------------------------------------------------------------------------------------------------
SA_RADII = [off_lattice(60), off_lattice(200)]


def sa_part(pm, out):
    for seed in range(200):
        rng = np.random.default_rng(9100 + seed)
        B, N = 2, 128
        xyz = np.stack([distinct_lattice(rng, N, (0, -32, -8), (64, 32, 8)) for _ in range(B)])
        feat = rng.standard_normal((B, 4, N)).astype(F32)
        res = {"sa_xyz": xyz, "sa_features": feat, "sa_radii": np.array(SA_RADII, F64)}
        torch.manual_seed(31)
        msg = pm.PointnetSAModuleMSG(npoint=32, radii=list(SA_RADII), nsamples=[8, 16], mlps=[[4, 8, 8], [4, 8, 16]], use_xyz=True)
        one = pm.PointnetSAModule(mlp=[4, 8, 16], npoint=None, radius=None, nsample=None, use_xyz=True)
        randomise(msg, rng)
        randomise(one, rng)
        state(msg, "sa_msg_", res)
        state(one, "sa_all_", res)
        for dtype, sfx in RUNS:
            with precision(dtype):
                for tag, ref in (("msg", msg), ("all", one)):
                    mod = copy.deepcopy(ref).to(dtype)
                    mod.eval()
                    with torch.no_grad():
                        res["sa_%s_out_eval%s" % (tag, sfx)] = mod(cast(xyz, dtype), cast(feat, dtype))[1].numpy()
                    mod.train()
                    with torch.no_grad():
                        new_xyz, o = mod(cast(xyz, dtype), cast(feat, dtype))
                    res["sa_%s_out_train%s" % (tag, sfx)] = o.numpy()
                    if tag == "msg":
                        res["sa_msg_new_xyz" + sfx] = new_xyz.numpy()
                    for k, v in mod.named_buffers():
                        res["sa_%s_after.%s%s" % (tag, k, sfx)] = v.detach().numpy().copy()
        if check_radii("sa seed %d" % seed):
            break
    else:
        raise SystemExit("sa_part: no seed meets condition (b)")
    out.update(res)


def fp_part(pm, out):
    rng = np.random.default_rng(9200)
    B, N, M = 2, 128, 32
    unknown = np.stack([distinct_lattice(rng, N, (0, -32, -8), (64, 32, 8)) for _ in range(B)])
    known = np.ascontiguousarray(unknown[:, ::4][:, :M])
    uf, kf = rng.standard_normal((B, 4, N)).astype(F32), rng.standard_normal((B, 8, M)).astype(F32)
    out.update(fp_unknown=unknown, fp_known=known, fp_unknow_feats=uf, fp_known_feats=kf)
    torch.manual_seed(32)
    ref = pm.PointnetFPModule(mlp=[8 + 4, 16, 16])
    randomise(ref, rng)
    state(ref, "fp_", out)
    for dtype, sfx in RUNS:
        with precision(dtype):
            mod = copy.deepcopy(ref).to(dtype)
            for mode in ("eval", "train"):
                mod.train(mode == "train")
                with torch.no_grad():
                    out["fp_out_%s%s" % (mode, sfx)] = mod(cast(unknown, dtype), cast(known, dtype), cast(uf, dtype), cast(kf, dtype)).numpy()


# ---- bb_* -------------------------------------------------------------------------------------------------------------------
BB_CFG = {'NAME': 'PointNet2MSG',
          'SA_CONFIG': {'NPOINTS': [64, 16, 8, 4],
                        'RADIUS': [[off_lattice(30), off_lattice(100)], [off_lattice(100), off_lattice(300)],
                                   [off_lattice(300), off_lattice(900)], [off_lattice(900), off_lattice(3000)]],
                        'NSAMPLE': [[16, 32], [16, 32], [16, 32], [16, 32]],
                        'MLPS': [[[8, 8, 16], [8, 8, 16]], [[16, 16, 32], [16, 24, 32]], [[32, 32, 32], [32, 32, 32]],
                                 [[32, 32, 64], [32, 48, 64]]]},
          'FP_MLPS': [[16, 16], [32, 32], [32, 32], [32, 32]]}


def bb_part(bb, out):
    for seed in range(200):
        rng = np.random.default_rng(9300 + seed)
        B, N = 2, 256
        pts = [np.concatenate([np.full((N, 1), b, F32), distinct_lattice(rng, N, (0, -32, -8), (64, 32, 8)),
                               rng.random((N, 1)).astype(F32)], axis=1) for b in range(B)]
        points = np.concatenate(pts).astype(F32)
        res = {"bb_points": points, "bb_cfg": np.array(json.dumps(BB_CFG))}
        torch.manual_seed(33)
        ref = bb.PointNet2MSG(to_attr(copy.deepcopy(BB_CFG)), input_channels=4)
        randomise(ref, rng)
        state(ref, "bb_", res)
        for dtype, sfx in RUNS:
            with precision(dtype):
                mod = copy.deepcopy(ref).to(dtype)
                for mode in ("eval", "train"):
                    mod.train(mode == "train")
                    with torch.no_grad():
                        bd = mod({'batch_size': B, 'points': cast(points, dtype)})
                    res["bb_point_features_%s%s" % (mode, sfx)] = bd['point_features'].numpy()
                res["bb_point_coords" + sfx] = bd['point_coords'].numpy()
        if check_radii("bb seed %d" % seed):
            break
    else:
        raise SystemExit("bb_part: no seed meets condition (b)")
    out.update(res)


# ---- ph_* -------------------------------------------------------------------------------------------------------------------
MEAN_SIZE = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]
PH_CFG = {'NAME': 'PointHeadBox', 'CLS_FC': [32, 32], 'REG_FC': [32, 32], 'CLASS_AGNOSTIC': False,
          'USE_POINT_FEATURES_BEFORE_FUSION': False,
          'TARGET_CONFIG': {'GT_EXTRA_WIDTH': [0.2, 0.2, 0.2], 'BOX_CODER': 'PointResidualCoder',
                            'BOX_CODER_CONFIG': {'use_mean_size': True, 'mean_size': MEAN_SIZE}},
          'LOSS_CONFIG': {'LOSS_REG': 'WeightedSmoothL1Loss',
                          'LOSS_WEIGHTS': {'point_cls_weight': 1.0, 'point_box_weight': 1.0, 'code_weights': [1.0] * 8}}}


def ph_part(coder_mod, ph, out):
    B, n, c = 2, 96, 24
    gt = np.zeros((B, 3, 8), F32)
    gt[0, 0] = [2.0, 0.0, 0.0, 3.9, 1.6, 1.56, 0.3, 1]
    gt[0, 1] = [5.5, -2.0, 0.25, 0.8, 0.6, 1.73, 1.2, 2]
    gt[1, 0] = [30.0, 10.0, 0.0, 1.76, 0.6, 1.73, -0.4, 3]            # far from every point: scene 1 has no foreground
    for seed in range(200):
        rng = np.random.default_rng(9400 + seed)
        coords = np.concatenate([np.concatenate([np.full((n, 1), b, F32), lattice(rng, n, (0, -24, -8), (56, 24, 8))], axis=1)
                                 for b in range(B)]).astype(F32)
        coords[0, 1:] = [2.0, 0.0, 0.0]                               # inside box 0
        coords[1, 1:] = [2.0, 0.0, 0.8125]                            # above box 0's top (0.78), inside the enlarged box (0.88)
        coords[2, 1:] = [5.5, -2.0, 0.25]                             # inside box 1 (class 2)
        coords[3, 1:] = [2.5, 0.25, -0.25]                            # inside box 0
        ext = gt.copy()
        ext[..., 3:6] += F32(0.2)
        margin = min(box_margin(coords[b * n:(b + 1) * n, 1:], np.concatenate([gt[b, :, :7], ext[b, :, :7]])) for b in range(B))
        if margin <= 1e-4:
            print("ph seed", seed, "refused: a box limit within %.1e of a point" % margin)
            continue
        feats = rng.standard_normal((B * n, c)).astype(F32)
        torch.manual_seed(34)
        ref = ph.PointHeadBox(num_class=3, input_channels=c, model_cfg=to_attr(copy.deepcopy(PH_CFG)))
        construct(ref, rng)
        centre(ref, lambda m: m({'batch_size': B, 'point_features': t(feats.copy()), 'point_coords': t(coords.copy()), 'gt_boxes': t(gt.copy())}))
        res = {"ph_coords": coords, "ph_features": feats, "ph_gt_boxes": gt, "ph_cfg": np.array(json.dumps(PH_CFG))}
        state(ref, "ph_", res)
        failed = None
        for dtype, sfx in RUNS:
            with precision(dtype):
                head = copy.deepcopy(ref).to(dtype)
                batch = lambda: {'batch_size': B, 'point_features': cast(feats, dtype), 'point_coords': cast(coords, dtype),
                                 'gt_boxes': cast(gt, dtype)}
                head.eval()
                with torch.no_grad():
                    bd = head(batch())
                res["ph_batch_cls_preds" + sfx] = bd['batch_cls_preds'].numpy()
                res["ph_batch_box_preds" + sfx] = bd['batch_box_preds'].numpy()
                res["ph_cls_scores_eval" + sfx] = bd['point_cls_scores'].numpy()
                head.train()
                with Margins(head) as mg:
                    head(batch())
                if dtype == torch.float64:
                    failed = mg.failed()
                loss_cls, tb1 = head.get_cls_layer_loss()
                loss_box, tb2 = head.get_box_layer_loss()
                (loss_cls + loss_box).backward()
                fr = head.forward_ret_dict
                res["ph_labels" + sfx] = fr['point_cls_labels'].numpy()
                res["ph_box_labels" + sfx] = fr['point_box_labels'].numpy()
                res["ph_cls_preds" + sfx] = fr['point_cls_preds'].detach().numpy()
                res["ph_box_preds" + sfx] = fr['point_box_preds'].detach().numpy()
                res["ph_loss_cls" + sfx], res["ph_loss_box" + sfx] = loss_cls.detach().numpy(), loss_box.detach().numpy()
                grads(head, "ph_", res, sfx)
        failed = failed or lucky(res, "ph_")
        if failed:
            print("ph seed", seed, "refused:", failed)
            continue
        break
    else:
        raise SystemExit("ph_part: no seed meets the conditions")
    labels = res["ph_labels"]
    print("ph: seed", seed, "labels", {int(v): int((labels == v).sum()) for v in np.unique(labels)}, "losses", float(res["ph_loss_cls"]),
          float(res["ph_loss_box"]), "relu margin %.2e" % mg.worst_relu)
    assert labels[0] == 1 and labels[1] == -1 and labels[2] == 2 and not labels[n:].any() and np.array_equal(res["ph_labels_f64"], labels)
    out.update(res)
    # the coder alone, with and without mean sizes
    boxes = rt.gt_rows(rng, 32, {1, 2, 3})
    boxes[0, 3:6] = 0                                                  # sizes below the clamp
    pts = (boxes[:, 0:3] + rng.standard_normal((32, 3)).astype(F32)).astype(F32)
    out.update(coder_boxes=boxes, coder_points=pts)
    for tag, kw in (("mean", {'use_mean_size': True, 'mean_size': MEAN_SIZE}), ("plain", {'use_mean_size': False})):
        coder = coder_mod.PointResidualCoder(**kw)
        for dtype, sfx in RUNS:
            with precision(dtype):
                classes = t(boxes[:, 7].astype(np.int64))
                codes = coder.encode_torch(cast(boxes[:, :7].copy(), dtype), cast(pts, dtype), classes)
                out["coder_%s_codes%s" % (tag, sfx)] = codes.numpy()
                out["coder_%s_decoded%s" % (tag, sfx)] = coder.decode_torch(codes, cast(pts, dtype), classes).numpy()


# ---- rh_* -------------------------------------------------------------------------------------------------------------------
RH_TARGET = dict(rt.BASE, ROI_PER_IMAGE=8)
RH_CFG = {'NAME': 'PointRCNNHead', 'CLASS_AGNOSTIC': True,
          'ROI_POINT_POOL': {'POOL_EXTRA_WIDTH': [0.0, 0.0, 0.0], 'NUM_SAMPLED_POINTS': 16, 'DEPTH_NORMALIZER': 70.0},
          'XYZ_UP_LAYER': [8, 8], 'CLS_FC': [16, 16], 'REG_FC': [16, 16], 'DP_RATIO': 0.0, 'USE_BN': False,
          'SA_CONFIG': {'NPOINTS': [8, 4, -1], 'RADIUS': [off_lattice(40), off_lattice(160), 100], 'NSAMPLE': [8, 8, 8],
                        'MLPS': [[8, 8, 8], [8, 8, 16], [16, 16, 16]]},
          'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                                   'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
                         'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                                  'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.85}},
          'TARGET_CONFIG': dict(RH_TARGET, BOX_CODER='ResidualCoder'),
          'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                          'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,
                                           'code_weights': [1.0] * 7}}}
RH_C = 8


def rh_scene(rng):
    """2 scenes x 160 points and 6 RoIs each: [fg with more than S points, fg, bg holding fewer than S points, a shifted bg,
    one far from every point (empty), a zero padding row]"""
    B, N = 2, 160
    gt = np.zeros((B, 3, 8), F32)
    gt[0, 0] = [10.0, 2.0, -1.0, 3.9, 1.6, 1.56, 0.3, 1]
    gt[0, 1] = [6.0, -3.0, -0.75, 0.8, 0.6, 1.73, 1.2, 2]
    gt[1, 0] = [12.0, -1.0, -0.75, 3.9, 1.6, 1.56, 0.0, 1]             # heading 0: its RoIs' canonical frames stay on the lattice
    gt[1, 1] = [7.0, 3.0, -0.75, 1.76, 0.6, 1.73, -0.7, 3]
    points, rois = [], np.zeros((B, 6, 7), F32)
    for b in range(B):
        car, small = gt[b, 0], gt[b, 1]
        # coordinates in general position: rotated lattice points would meet the sampling's decisions with exact ties, which
        # the rounding of the canonical transformation then breaks one way in the reference and another on the device
        near = lambda g, n, w: (g[0:3] + rng.uniform(-1, 1, (n, 3)) * (np.array(w) / 8.0)).astype(F32)
        pts = np.concatenate([near(car, 70, (12, 5, 5)), near(small, 20, (3, 3, 6)),
                              rng.uniform((0, -5, -2), (20, 5, 0), (N - 90, 3)).astype(F32)])
        points.append(np.concatenate([np.full((N, 1), b, F32), pts], axis=1))
        rois[b, 0] = car[:7] + np.array([0.125, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], F32)
        rois[b, 1] = small[:7] + np.array([0.0, 0.0, 0.0, 0.05, 0.05, 0.0, 0.0], F32)
        rois[b, 2] = car[:7] + np.array([1.25, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0], F32)
        rois[b, 3] = small[:7] + np.array([0.25, 0.25, 0.0, 0.0, 0.0, 0.0, 0.2 if b == 0 else 0.0], F32)
        rois[b, 4] = [60.0, 30.0, 5.0, 2.0, 2.0, 2.0, 0.5]
    return np.concatenate(points).astype(F32), rois, gt


def rh_part(rh, out):
    B = 2
    for seed in range(400):
        rng = np.random.default_rng(9500 + seed)
        coords, rois, gt = rh_scene(rng)
        N = len(coords) // B
        S = RH_CFG['ROI_POINT_POOL']['NUM_SAMPLED_POINTS']
        margin = min(box_margin(coords[b * N:(b + 1) * N, 1:], rois[b]) for b in range(B))
        inside = np.array([[rp.in_box(coords[b * N:(b + 1) * N, 1:], rois[b, m], rp.MARGIN_GPU, 1)[0].sum() for m in range(6)] for b in range(B)])
        if margin <= 1e-4 or not ((inside[:, 0] > S).all() and (inside[:, 4:] == 0).all()
                                  and ((inside[:, 1:4] > 0) & (inside[:, 1:4] < S)).any(axis=1).all()):
            print("rh seed", seed, "refused: margin %.1e, points inside" % margin, inside.tolist())
            continue
        feats = rng.standard_normal((len(coords), RH_C)).astype(F32)
        scores = rng.random(len(coords)).astype(F32)
        roi_scores = rng.random((B, 6)).astype(F32)
        roi_labels = np.array([[1, 2, 1, 2, 1, 1], [1, 3, 1, 3, 1, 1]], np.int64)
        np.random.seed(500 + seed)
        torch.manual_seed(500 + seed)
        tg, _, targets = rt.run_targets('rh', RH_TARGET, rois, roi_scores, roi_labels, gt)
        res = {"rh_coords": coords, "rh_features": feats, "rh_scores": scores, "rh_cfg": np.array(json.dumps(RH_CFG)),
               "rh_c_in": np.int32(RH_C)}
        res.update({"rh_" + k: v for k, v in tg.items() if k not in ('case', 'cfg')})
        torch.manual_seed(35)
        ref = rh.PointRCNNHead(input_channels=RH_C, model_cfg=to_attr(copy.deepcopy(RH_CFG)), num_class=1)
        construct(ref, rng)
        with torch.no_grad():
            for seq in (ref.xyz_up_layer, ref.merge_down_layer):        # Conv2d + ReLU without BatchNorm: small weights, large biases
                for m in seq:
                    if isinstance(m, nn.Conv2d):
                        m.weight.mul_(0.02)
                        b = 1.0 + 0.5 * torch.rand(m.bias.shape)
                        b[::5] *= -1
                        m.bias.copy_(b)

        def train_pass(m):
            m.assign_targets = lambda bd: {k: v.clone() for k, v in targets.items()}
            m({'batch_size': B, 'rois': t(rois.copy()), 'roi_scores': t(roi_scores.copy()), 'roi_labels': t(roi_labels.copy()),
               'gt_boxes': t(gt.copy()), 'point_coords': t(coords.copy()), 'point_features': t(feats.copy()), 'point_cls_scores': t(scores.copy())})
            del m.__dict__['assign_targets']
        centre(ref, train_pass)
        state(ref, "rh_", res)
        failed = None
        for dtype, sfx in RUNS:
            with precision(dtype):
                head = copy.deepcopy(ref).to(dtype)
                batch = lambda: {'batch_size': B, 'rois': cast(rois, dtype), 'roi_scores': cast(roi_scores, dtype), 'roi_labels': t(roi_labels.copy()),
                                 'gt_boxes': cast(gt, dtype), 'point_coords': cast(coords, dtype), 'point_features': cast(feats, dtype),
                                 'point_cls_scores': cast(scores, dtype)}
                head.eval()
                with torch.no_grad():
                    res["rh_pooled_eval" + sfx] = head.roipool3d_gpu(batch()).numpy()
                    bd = head(batch())
                res["rh_batch_cls_preds" + sfx], res["rh_batch_box_preds" + sfx] = bd['batch_cls_preds'].numpy(), bd['batch_box_preds'].numpy()
                head.train()
                head.assign_targets = lambda bd: {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in targets.items()}
                bd = batch()
                levels = []                                    # the SA stack's outputs, to tell the stack from the fc layers
                hooks = [m.register_forward_hook(lambda mod, args, o: levels.append(o[1].detach().numpy().copy())) for m in head.SA_modules]
                with Margins(head, sys.modules["pcdet_ref.ops.pointnet2.pointnet2_batch.pointnet2_modules"]) as mg:
                    head(bd)
                for k, h in enumerate(hooks):
                    h.remove()
                    res["rh_sa%d_train%s" % (k, sfx)] = levels[k]
                if dtype == torch.float64:
                    failed = mg.failed()
                with torch.no_grad():
                    res["rh_pooled_train" + sfx] = head.roipool3d_gpu(bd).numpy()
                loss, tb = head.get_loss()
                loss.backward()
                fr = head.forward_ret_dict
                res["rh_rcnn_cls" + sfx], res["rh_rcnn_reg" + sfx] = fr['rcnn_cls'].detach().numpy(), fr['rcnn_reg'].detach().numpy()
                for k in ('rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner'):
                    res["rh_" + k + sfx] = np.asarray(tb[k], F64 if dtype == torch.float64 else F32)
                res["rh_loss" + sfx] = loss.detach().numpy()
                grads(head, "rh_", res, sfx)
        ok_radii, ok_fps = check_radii("rh seed %d" % seed), check_samplings("rh seed %d" % seed)
        failed = failed or lucky(res, "rh_")
        if failed or not ok_radii or not ok_fps:
            print("rh seed", seed, "refused:", failed or "a distance within 1e-3 of a radius, or a sampling decision within 1e-4")
            continue
        break
    else:
        raise SystemExit("rh_part: no seed meets the conditions")
    print("rh: seed", seed, "points inside", inside.tolist(), "fg", int((res["rh_t_reg_valid_mask"] > 0).sum()), "cls labels",
          res["rh_t_rcnn_cls_labels"].reshape(-1).tolist(), "losses", {k: float(res["rh_" + k]) for k in ('rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner')},
          "relu margin %.2e win margin %.2e" % (mg.worst_relu, mg.worst_win))
    assert (res["rh_t_reg_valid_mask"] > 0).any()
    out.update(res)


def state_dict_part(root, bb, ph, rh):
    y = model_yaml(root, "kitti_models/pointrcnn.yaml")
    model, names = y["MODEL"], y["CLASS_NAMES"]
    backbone = bb.PointNet2MSG(to_attr(copy.deepcopy(model["BACKBONE_3D"])), input_channels=4)
    point = ph.PointHeadBox(num_class=3, input_channels=backbone.num_point_features, model_cfg=to_attr(copy.deepcopy(model["POINT_HEAD"])),
                            predict_boxes_when_training=True)
    head = rh.PointRCNNHead(input_channels=backbone.num_point_features, model_cfg=to_attr(copy.deepcopy(model["ROI_HEAD"])), num_class=1)
    out = {"PointNet2MSG": shapes(backbone), "PointHeadBox": shapes(point), "PointRCNNHead": shapes(head)}
    # the whole detector: the reference's module_topology keeps backbone_3d, point_head, roi_head of this config, in that order
    out["PointRCNN"] = shapes(backbone, "backbone_3d.") + shapes(point, "point_head.") + shapes(head, "roi_head.")
    out["config"] = {"MODEL": model, "dataset": {"class_names": names, "num_point_features": 4}}
    write_state_dict("pointrcnn_state_dict.json", out)


def main():
    root = reference_root()
    pm, bb, coder_mod, ph, rh = load_reference(root)
    out = {}
    sa_part(pm, out)
    fp_part(pm, out)
    bb_part(bb, out)
    ph_part(coder_mod, ph, out)
    rh_part(rh, out)
    path = os.path.join(HERE, "pointrcnn.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < 1 << 20
    state_dict_part(root, bb, ph, rh)


if __name__ == "__main__":
    main()
