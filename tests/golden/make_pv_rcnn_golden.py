#!/usr/bin/env python
"""Generates tests/golden/pv_rcnn.npz and tests/golden/pv_rcnn_state_dict.json from the REFERENCE's own
pointnet2_stack/pointnet2_modules.py, voxel_set_abstraction.py, point_head_simple.py and pvrcnn_head.py, imported from where
they lie and run on the CPU in float32.

    python tests/golden/make_pv_rcnn_golden.py <checkout of the reference>

The `pointnet2_stack_cuda` extension is a stub over numpy restatements (stack_sa_restatement.py: ball query, farthest-point
sampling; the grouping entries are gathers), roiaware_pool3d_utils.points_in_boxes_gpu likewise; the loading and the CPU
patches are reference_loader.py's.  Nothing of the reference is copied; what is committed is data.  The grouping backward
adds in float32, as the reference's kernel does with its float atomicAdd (in an order the hardware picks; the stub takes the ascending one): a float64 accumulation there would
make the fixture's feature gradient more accurate than any float32 run of the reference, and the tests measure the device
against the error of such a run.

pv_rcnn.npz
  sa_*     one StackSAModuleMSG with two scales (C_in 16 -> [16, 16] at nsample 16, -> [64, 32] at nsample 32) over 2 scenes:
           inputs, parameters and buffers, the train-mode output, the gradients of sum(out * grad_out) for every parameter
           and for `features`, the running statistics after that step, the eval-mode output.
  bev_*    interpolate_from_bev_features on a (2, 8, 6, 5) map: keypoints inside, on cell corners and beyond every border.
  vsa_*    VoxelSetAbstraction (bev, raw_points, x_conv1, x_conv2; NUM_KEYPOINTS 64; scene 1 has 32 points): keypoint rows,
           both feature tensors in train and eval mode.
  head_*   PVRCNNHead (GRID_SIZE 3, DP_RATIO 0) on given RoIs: pooled features and both predictions in train and eval mode,
           eval's decoded batch_cls_preds / batch_box_preds.
  point_*  PointHeadSimple: labels and loss on given keypoints and boxes (one point lies only in the enlarged box).

Coordinates lie on the 1/8 lattice: squared distances are exact in float32 and no query depends on the contraction mode.  The
farthest-point sampling meets ties there.  The reference samples each scene with its BATCH kernel (block size
opt_n_threads(n)); a stacked launch follows the reference's STACKED kernel (block size 1024), whose tree orders equal distances
differently unless n is a power of two (stack_sa_restatement.py).  The scenes of vsa_* hold 256 and 32 points, and the
generator checks that both rules give the same keypoints there.

Two conditions are checked in float64 and the generator fails when one does not hold (sa_part then tries the next seed):
 (a) no argmax or ReLU mask of the sa_* module can flip at float32 precision: every (centre, channel) winner of y2 beats the next
     distinct value of its row by WIN_MARGIN of max |y2|, and every first-layer pre-activation s1 y1 + t1 and every pooled
     pre-ReLU output lies further than 1e-3 of its tensor's largest magnitude from zero.  Random parameters cannot meet the
     second part (hundreds of 700 000 slots fall inside any such band), so the module's parameters are CONSTRUCTED: the
     source features are +-(1 .. 2) per channel, the feature columns of the first conv are diagonal, so y1 is bimodal with a gap
     around the BatchNorm's zero crossing; the second BatchNorm has |bias| well above |weight| times the spread, weights
     of both signs.  WIN_MARGIN = 2e-5: an fma chain of 64 float32 terms is within 64 x 2^-24 = 4e-6 of its exact value
     relative to the sum of magnitudes, which is below 5 max |y2|.
 (b) no centre-to-point distance of any ball query in the file lies within 1e-3 of the query's radius.

pv_rcnn_state_dict.json: keys and shapes, in order, of the reference's PVRCNNHead, VoxelSetAbstraction and PointHeadSimple for
kitti_models/pv_rcnn.yaml, of the whole PVRCNN on the settings of second_state_dict.json (its reduced grid and cut 2D
backbone, three classes) in the reference's module order, and the config used.
"""
import copy
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import stack_sa_restatement as rs  # noqa: E402
from make_voxel_rcnn_golden import PCR, VOXEL, sparse_level  # noqa: E402
from reference_loader import (MODEL_UTILS, ROI_HEAD, as_np as _np, cpu_torch, extension_stubs, load, model_yaml,  # noqa: E402
                              randomise, reference_root, second_settings, shapes, state, write_state_dict)
from pdanet_amd.config import to_attr  # noqa: E402

F32, I32 = np.float32, np.int32
WIN_MARGIN = 2e-5
t = torch.from_numpy
QUERIES = []                     # (radius, new_xyz, new_cnt, xyz, cnt) of every ball query made, for condition (b)


class Stub(types.ModuleType):
    def __init__(self):
        super().__init__("pointnet2_stack_cuda")

    @staticmethod
    def ball_query_wrapper(B, M, radius, nsample, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, idx):
        QUERIES.append((float(radius), _np(new_xyz).copy(), _np(new_xyz_batch_cnt).copy(), _np(xyz).copy(), _np(xyz_batch_cnt).copy()))
        rs.ball_query(radius, nsample, _np(new_xyz), _np(new_xyz_batch_cnt), _np(xyz), _np(xyz_batch_cnt), _np(idx))
        return 1

    @staticmethod
    def group_points_wrapper(B, M, C, nsample, features, features_batch_cnt, idx, idx_batch_cnt, out):
        rows = _np(idx).astype(np.int64) + np.repeat(rs.starts(_np(features_batch_cnt)), _np(idx_batch_cnt))[:, None]
        _np(out)[...] = _np(features)[rows].transpose(0, 2, 1)
        return 1

    @staticmethod
    def group_points_grad_wrapper(B, M, C, N, nsample, grad_out, idx, idx_batch_cnt, features_batch_cnt, grad_features):
        rows = _np(idx).astype(np.int64) + np.repeat(rs.starts(_np(features_batch_cnt)), _np(idx_batch_cnt))[:, None]
        acc = np.zeros((N, C), F32)                # float32 adds, one after the other in (centre, slot) order, as ONE order the
        np.add.at(acc, rows.reshape(-1), _np(grad_out).transpose(0, 2, 1).reshape(-1, C))      # kernel's float atomics can take
        _np(grad_features)[...] = acc
        return 1

    @staticmethod
    def farthest_point_sampling_wrapper(B, N, npoint, xyz, temp, output):
        for b in range(B):
            _np(output)[b] = np.maximum(rs.fps(_np(xyz)[b], npoint), 0)
        return 1


def load_reference(root):
    """-> the reference's modules as pcdet_ref.*"""
    cpu_torch()
    stack = "ops.pointnet2.pointnet2_stack."
    load(root, "pcdet_ref", MODEL_UTILS + ROI_HEAD + [stack + "pointnet2_utils", "models.dense_heads.point_head_template"],
         stubs=extension_stubs({stack + "pointnet2_stack_cuda": Stub()}))
    return load(root, "pcdet_ref", [stack + "pointnet2_modules", "models.backbones_3d.pfe.voxel_set_abstraction",
                                    "models.dense_heads.point_head_simple", "models.roi_heads.pvrcnn_head"])


def check_radii(what):
    """condition (b) over the queries recorded since the last call"""
    worst = np.inf
    for radius, new_xyz, new_cnt, xyz, cnt in QUERIES:
        ps, qs = rs.starts(cnt), rs.starts(new_cnt)
        for b in range(len(cnt)):
            p = xyz[ps[b]:ps[b] + cnt[b]].astype(np.float64)
            q = new_xyz[qs[b]:qs[b] + new_cnt[b]].astype(np.float64)
            if len(p) and len(q):
                d = np.sqrt(((q[:, None, :] - p[None, :, :]) ** 2).sum(-1))
                worst = min(worst, float(np.abs(d - radius).min()))
    print("%s: %d ball queries, the nearest distance to a radius is %.4f" % (what, len(QUERIES), worst))
    assert worst > 1e-3, "%s: a distance lies within 1e-3 of a radius" % what
    del QUERIES[:]


def lattice(rng, n, lo=(0, -32, -16), hi=(64, 32, 16), step=8):
    return np.stack([rng.integers(lo[k], hi[k], n) for k in range(3)], axis=1).astype(F32) / step


# radii whose squares fall between two lattice values k / 64
SA_RADII = [float(np.sqrt(100.5 / 64)), float(np.sqrt(400.5 / 64))]


def sa_inputs(rng):
    cnt, new_cnt = np.array([220, 180], I32), np.array([157, 146], I32)
    xyz = []
    for n in cnt:                                   # half of a scene in a dense cube: balls with more than nsample hits
        xyz.append(np.concatenate([lattice(rng, n // 2), lattice(rng, n - n // 2, (16, -8, -8), (32, 8, 8))]))
    xyz = np.concatenate(xyz)
    new_xyz = np.concatenate([lattice(rng, new_cnt[0]), lattice(rng, new_cnt[1])])
    new_xyz[:4] += 40                               # empty balls
    new_xyz[new_cnt[0]:new_cnt[0] + 3] -= 40
    sign = rng.integers(0, 2, (len(xyz), 16)) * 2 - 1
    feat = (sign * (1.0 + rng.random((len(xyz), 16)))).astype(F32)
    grad_out = rng.standard_normal((int(new_cnt.sum()), 16 + 32)).astype(F32)
    return dict(sa_xyz=xyz, sa_xyz_cnt=cnt, sa_new_xyz=new_xyz, sa_new_cnt=new_cnt, sa_features=feat, sa_grad_out=grad_out)


def sa_construct(mod, rng):
    """The parameters of condition (a), see the module docstring."""
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    r = lambda *s: torch.rand(*s, generator=g)
    with torch.no_grad():
        for mlp in mod.mlps:
            conv1, bn1, _, conv2, bn2, _ = mlp
            c1, c2 = conv1.out_channels, conv2.out_channels
            w = torch.zeros(c1, 19)
            w[:, :3] = (r(c1, 3) - 0.5) * 0.04
            w[torch.arange(c1), 3 + torch.arange(c1) % 16] = (0.8 + 0.4 * r(c1)) * (torch.randint(0, 2, (c1,), generator=g) * 2 - 1)
            conv1.weight.copy_(w.view(c1, 19, 1, 1))
            bn1.weight.copy_((0.6 + 0.6 * r(c1)) * (torch.randint(0, 2, (c1,), generator=g) * 2 - 1))
            bn1.bias.copy_(bn1.weight.abs() * 0.2 * (torch.randint(0, 2, (c1,), generator=g) * 2 - 1))
            bn1.running_mean.copy_((r(c1) - 0.5) * 0.1)
            bn1.running_var.copy_(1.5 + r(c1))
            conv2.weight.copy_(torch.randn(c2, c1, 1, 1, generator=g) / c1 ** 0.5)
            bn2.weight.copy_((0.1 + 0.1 * r(c2)) * (torch.randint(0, 2, (c2,), generator=g) * 2 - 1))
            bias = 1.2 + 0.4 * r(c2)
            bias[::5] *= -1                         # every fifth channel is dead behind its ReLU
            bn2.bias.copy_(bias)
            bn2.running_mean.copy_((r(c2) - 0.5) * 0.2)
            bn2.running_var.copy_(0.6 + 0.4 * r(c2))    # y2's variance is about 0.5: the eval statistics stay near the batch's


@torch.no_grad()
def sa_margins(mod, inp):
    """Condition (a) in float64, in train and eval statistics.  -> None, or what failed."""
    m64 = copy.deepcopy(mod).double()
    xyz, new_xyz = t(inp['sa_xyz']), t(inp['sa_new_xyz'])
    feat = t(inp['sa_features']).double()
    for k, grouper in enumerate(m64.groupers):
        idx = np.zeros((len(new_xyz), grouper.nsample), I32)
        rs.ball_query(grouper.radius, grouper.nsample, inp['sa_new_xyz'], inp['sa_new_cnt'], inp['sa_xyz'], inp['sa_xyz_cnt'], idx)
        empty = t(idx[:, 0] < 0)
        rows = t(np.where(idx[:, :1] < 0, 0, idx).astype(np.int64) + np.repeat(rs.starts(inp['sa_xyz_cnt']), inp['sa_new_cnt'])[:, None])
        rel = (xyz[rows] - new_xyz[:, None, :]).double()
        x = torch.cat([rel, feat[rows]], dim=-1).masked_fill(empty[:, None, None], 0)            # (M, ns, 19)
        conv1, bn1, _, conv2, bn2, _ = m64.mlps[k]
        y1 = x @ conv1.weight[:, :, 0, 0].t()
        for train in (True, False):
            flat = y1.reshape(-1, y1.shape[-1])
            mean, var = (flat.mean(0), flat.var(0, unbiased=False)) if train else (bn1.running_mean, bn1.running_var)
            a1 = (y1 - mean) / torch.sqrt(var + bn1.eps) * bn1.weight + bn1.bias
            if float(a1.abs().min()) <= 1e-3 * float(a1.abs().max()):
                return "scale %d train %s: a first-layer pre-activation at %.2e of the largest" % (k, train, float(a1.abs().min() / a1.abs().max()))
            y2 = torch.relu(a1) @ conv2.weight[:, :, 0, 0].t()                                  # (M, ns, C2)
            flat = y2.reshape(-1, y2.shape[-1])
            mean, var = (flat.mean(0), flat.var(0, unbiased=False)) if train else (bn2.running_mean, bn2.running_var)
            a2 = (y2 - mean) / torch.sqrt(var + bn2.eps) * bn2.weight + bn2.bias
            pooled = a2.max(dim=1)[0]
            if float(pooled.abs().min()) <= 1e-3 * float(pooled.abs().max()):
                return "scale %d train %s: a pooled pre-ReLU output at %.2e of the largest" % (k, train, float(pooled.abs().min() / pooled.abs().max()))
            signed = y2 * torch.sign(bn2.weight)                                                 # the winner is the largest of these
            top = signed.max(dim=1, keepdim=True)[0]
            gap = torch.where(signed < top, top - signed, torch.full_like(signed, float('inf'))).min(dim=1)[0]
            if float(gap.min()) <= WIN_MARGIN * float(y2.abs().max()):
                return "scale %d train %s: a winner leads by %.2e of max |y2|" % (k, train, float(gap.min() / y2.abs().max()))
    return None


def sa_part(pm, out):
    for seed in range(2000):
        rng = np.random.default_rng(7000 + seed)
        inp = sa_inputs(rng)
        torch.manual_seed(21)
        mod = pm.StackSAModuleMSG(radii=list(SA_RADII), nsamples=[16, 32], mlps=[[16, 16, 16], [16, 64, 32]], use_xyz=True,
                                  pool_method='max_pool')
        sa_construct(mod, rng)
        failed = sa_margins(mod, inp)
        if failed is None:
            break
        print("sa seed", seed, "refused:", failed)
    else:
        raise SystemExit("sa_part: no seed meets condition (a)")
    print("sa: seed", seed, "meets condition (a)")
    out.update(inp)
    out["sa_radii"] = np.array(SA_RADII, np.float64)
    state(mod, "sa_", out)
    args = dict(xyz=t(inp['sa_xyz']), xyz_batch_cnt=t(inp['sa_xyz_cnt']), new_xyz=t(inp['sa_new_xyz']),
                new_xyz_batch_cnt=t(inp['sa_new_cnt']))
    mod.eval()
    with torch.no_grad():
        out["sa_out_eval"] = mod(features=t(inp['sa_features'].copy()), **args)[1].numpy()
    mod.train()
    f = t(inp['sa_features'].copy()).requires_grad_(True)
    res = mod(features=f, **args)[1]
    (res * t(inp['sa_grad_out'])).sum().backward()
    out["sa_out_train"] = res.detach().numpy()
    out["sa_grad_features"] = f.grad.numpy()
    for k, p in mod.named_parameters():
        out["sa_grad." + k] = p.grad.numpy().copy()
    for k, v in mod.named_buffers():
        out["sa_after." + k] = v.detach().numpy().copy()
    for k, grouper in enumerate(mod.groupers):
        idx = np.zeros((len(inp['sa_new_xyz']), grouper.nsample), I32)
        rs.ball_query(grouper.radius, grouper.nsample, inp['sa_new_xyz'], inp['sa_new_cnt'], inp['sa_xyz'], inp['sa_xyz_cnt'], idx)
        empty, short = idx[:, 0] < 0, (idx[:, -1] == idx[:, 0]) & (idx[:, 0] >= 0)
        print("sa scale", k, "centres", len(idx), "empty balls", int(empty.sum()), "short lists", int(short.sum()), "full lists",
              int((~empty & ~short).sum()), "dead output channels", int((out["sa_out_train"][:, 16 * k:16 + 32 * k] == 0).all(0).sum()))
        assert empty.any() and short.any() and (~empty & ~short).any()
    check_radii("sa")


def bev_part(vsa_mod, rng, out):
    B, C, H, W = 2, 8, 6, 5
    bev = rng.standard_normal((B, C, H, W)).astype(F32)
    stride, pcr, voxel = 2, [0.0, -1.5, -1.0, 2.5, 1.5, 1.0], [0.25, 0.25, 0.25]     # x = 2 px, y = 2 (py + 1.5) in map cells
    xs = np.concatenate([rng.uniform(0.1, 2.3, 12), np.arange(0, 5) * 0.5, [-0.3, -0.6, 2.45, 2.9, 1.0, 1.0, 2.0, -0.5]])
    ys = np.concatenate([rng.uniform(-1.4, 1.4, 12), np.arange(0, 5) * 0.5 - 1.5, [0.0, 0.2, 0.1, 0.3, -1.7, 1.9, 1.0, 1.6]])
    kp = np.stack([rng.integers(0, B, len(xs)).astype(np.float64), xs, ys, np.zeros(len(xs))], axis=1).astype(F32)
    kp = kp[np.argsort(kp[:, 0], kind='stable')]
    grad_out = rng.standard_normal((len(kp), C)).astype(F32)
    obj = types.SimpleNamespace(point_cloud_range=pcr, voxel_size=voxel)
    b = t(bev.copy()).requires_grad_(True)
    res = vsa_mod.VoxelSetAbstraction.interpolate_from_bev_features(obj, t(kp), b, B, stride)
    (res * t(grad_out)).sum().backward()
    out.update(bev_map=bev, bev_keypoints=kp, bev_grad_out=grad_out, bev_out=res.detach().numpy(), bev_grad_map=b.grad.numpy(),
               bev_stride=np.int32(stride), bev_pcr=np.array(pcr), bev_voxel=np.array(voxel))


VSA_CFG = {
    'NAME': 'VoxelSetAbstraction', 'POINT_SOURCE': 'raw_points', 'NUM_KEYPOINTS': 64, 'NUM_OUTPUT_FEATURES': 32,
    'SAMPLE_METHOD': 'FPS', 'FEATURES_SOURCE': ['bev', 'x_conv1', 'x_conv2', 'raw_points'],
    'SA_LAYER': {
        'raw_points': {'MLPS': [[16, 16], [16, 16]], 'POOL_RADIUS': [float(np.sqrt(60.5 / 64)), float(np.sqrt(150.5 / 64))], 'NSAMPLE': [16, 16]},
        'x_conv1': {'DOWNSAMPLE_FACTOR': 1, 'MLPS': [[16, 16], [16, 16]], 'POOL_RADIUS': [float(np.sqrt(60.5 / 64)), float(np.sqrt(150.5 / 64))],
                    'NSAMPLE': [16, 16]},
        'x_conv2': {'DOWNSAMPLE_FACTOR': 2, 'MLPS': [[32, 32], [32, 32]], 'POOL_RADIUS': [float(np.sqrt(150.5 / 64)), float(np.sqrt(300.5 / 64))],
                    'NSAMPLE': [16, 32]}}}
VSA_BEV = (16, 8, 8)             # channels, H, W of spatial_features at stride 4 on the fixture's 32 x 32 grid


def vsa_part(vsa_mod, rng, out):
    B, counts = 2, [256, 32]            # powers of two: the batch and the stacked sampling kernels break ties alike
    pts = []
    for b, n in enumerate(counts):      # raw points on the lattice, distinct, one intensity column
        xyz = np.unique(lattice(rng, n + 40), axis=0)
        xyz = xyz[rng.permutation(len(xyz))[:n]]
        assert len(xyz) == n
        pts.append(np.concatenate([np.full((n, 1), b), xyz, rng.random((n, 1))], axis=1))
    points = np.concatenate(pts).astype(F32)
    levels = {}
    for name, stride, per_scene, c in (('x_conv1', 1, [400, 250], 16), ('x_conv2', 2, [300, 200], 32)):
        ind, feat, shape = sparse_level(rng, stride, per_scene, c)
        levels[name] = (ind, feat, shape)
        out["vsa_%s_indices" % name], out["vsa_%s_features" % name] = ind, feat
        out["vsa_%s_spatial_shape" % name] = np.array(shape, I32)
    bev = rng.standard_normal((B,) + VSA_BEV).astype(F32)
    out.update(vsa_points=points, vsa_bev=bev, vsa_cfg=np.array(json.dumps(VSA_CFG)))
    torch.manual_seed(13)
    mod = vsa_mod.VoxelSetAbstraction(to_attr(copy.deepcopy(VSA_CFG)), VOXEL, PCR, num_bev_features=VSA_BEV[0], num_rawpoint_features=4)
    randomise(mod, rng)
    state(mod, "vsa_", out)

    def batch():
        feats = {k: types.SimpleNamespace(indices=t(v[0]), features=t(v[1].copy())) for k, v in levels.items()}
        return {'batch_size': B, 'points': t(points.copy()), 'multi_scale_3d_features': feats, 'spatial_features': t(bev.copy()),
                'spatial_features_stride': 4}

    for mode in ("eval", "train"):
        mod.train(mode == "train")
        with torch.no_grad():
            bd = mod(batch())
        out["vsa_before_fusion_" + mode] = bd['point_features_before_fusion'].numpy()
        out["vsa_point_features_" + mode] = bd['point_features'].numpy()
    out["vsa_point_coords"] = bd['point_coords'].numpy()
    rows = []                                       # the keypoints as rows of `points`
    for b, n in enumerate(counts):
        start = sum(counts[:b])
        first = rs.fps(points[start:start + n, 1:4], min(n, 64))
        assert np.array_equal(first, rs.fps(points[start:start + n, 1:4], min(n, 64), block=1024))
        rows.append(start + first[np.arange(64) % len(first)])
    out["vsa_keypoint_rows"] = np.stack(rows).astype(np.int64)
    assert np.array_equal(points[out["vsa_keypoint_rows"].reshape(-1), 1:4], out["vsa_point_coords"][:, 1:4])
    print("vsa: point_features", out["vsa_point_features_train"].shape, "before fusion", out["vsa_before_fusion_train"].shape)
    check_radii("vsa")


HEAD_CFG = {
    'NAME': 'PVRCNNHead', 'CLASS_AGNOSTIC': True, 'SHARED_FC': [32, 32], 'CLS_FC': [32, 32], 'REG_FC': [32, 32], 'DP_RATIO': 0.0,
    'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                             'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
                   'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 1024,
                            'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.7}},
    'ROI_GRID_POOL': {'GRID_SIZE': 3, 'MLPS': [[16, 16], [32, 16]], 'POOL_RADIUS': [float(np.sqrt(100.5 / 64)), float(np.sqrt(250.5 / 64))],
                      'NSAMPLE': [16, 16], 'POOL_METHOD': 'max_pool'},
    'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5, 'SAMPLE_ROI_BY_EACH_CLASS': True,
                      'CLS_SCORE_TYPE': 'roi_iou', 'CLS_FG_THRESH': 0.75, 'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1,
                      'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55},
    'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                    'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,
                                     'code_weights': [1.0] * 7}},
}
HEAD_C_IN = 24


def head_part(head_mod, rng, out):
    B, n_roi, per_scene = 2, 5, [150, 110]
    coords = np.concatenate([np.concatenate([np.full((n, 1), b, F32), lattice(rng, n)], axis=1) for b, n in enumerate(per_scene)]).astype(F32)
    feats = rng.standard_normal((len(coords), HEAD_C_IN)).astype(F32)
    scores = rng.random(len(coords)).astype(F32)
    rois = np.zeros((B, n_roi, 7), F32)
    rois[..., 0] = rng.integers(8, 56, (B, n_roi)) / 8
    rois[..., 1] = rng.integers(-24, 24, (B, n_roi)) / 8
    rois[..., 2] = rng.integers(-8, 8, (B, n_roi)) / 8
    rois[..., 3:6] = rng.integers(1, 3, (B, n_roi, 3)) * 3           # sizes 3 or 6: the grid points stay on the lattice
    rois[1, -1] = 0                                                  # a zero-padded RoI row
    out.update(head_rois=rois, head_point_coords=coords, head_point_features=feats, head_point_cls_scores=scores,
               head_cfg=np.array(json.dumps(HEAD_CFG)), head_c_in=np.int32(HEAD_C_IN))
    torch.manual_seed(12)
    head = head_mod.PVRCNNHead(input_channels=HEAD_C_IN, model_cfg=to_attr(copy.deepcopy(HEAD_CFG)), num_class=1)
    randomise(head, rng)
    with torch.no_grad():                               # the reference's std 0.001 would leave the predictions at zero
        head.cls_layers[-1].weight.normal_(0, 0.3, generator=torch.Generator().manual_seed(5))
        head.reg_layers[-1].weight.normal_(0, 0.1, generator=torch.Generator().manual_seed(6))
    state(head, "head_", out)

    def batch():
        return {'batch_size': B, 'rois': t(rois.copy()), 'roi_scores': torch.zeros(B, n_roi), 'roi_labels': torch.ones(B, n_roi, dtype=torch.long),
                'point_coords': t(coords.copy()), 'point_features': t(feats.copy()), 'point_cls_scores': t(scores.copy())}

    head.eval()
    with torch.no_grad():
        out["head_pooled_eval"] = head.roi_grid_pool(batch()).numpy()
        bd = head(batch())
        out["head_batch_cls_preds"], out["head_batch_box_preds"] = bd['batch_cls_preds'].numpy(), bd['batch_box_preds'].numpy()
    head.train()
    with torch.no_grad():
        pooled = head.roi_grid_pool(batch())
        shared = head.shared_fc_layer(pooled.permute(0, 2, 1).contiguous().view(pooled.shape[0], -1, 1))
        out["head_pooled_train"] = pooled.numpy()
        out["head_rcnn_cls_train"] = head.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1).numpy()
        out["head_rcnn_reg_train"] = head.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1).numpy()
    print("head: pooled", out["head_pooled_train"].shape, "nonzero share", float((out["head_pooled_train"] != 0).mean()))
    check_radii("head")


POINT_CFG = {'NAME': 'PointHeadSimple', 'CLS_FC': [32, 32], 'CLASS_AGNOSTIC': True, 'USE_POINT_FEATURES_BEFORE_FUSION': True,
             'TARGET_CONFIG': {'GT_EXTRA_WIDTH': [0.2, 0.2, 0.2]},
             'LOSS_CONFIG': {'LOSS_REG': 'smooth-l1', 'LOSS_WEIGHTS': {'point_cls_weight': 1.0}}}


def point_part(point_mod, rng, out):
    B, n, c = 2, 96, 24
    gt = np.zeros((B, 3, 8), F32)
    gt[0, 0] = [2.0, 0.0, 0.0, 3.0, 1.5, 1.5, 0.3, 1]
    gt[0, 1] = [5.5, -2.0, 0.25, 1.0, 0.75, 1.75, 1.2, 2]
    gt[1, 0] = [3.0, 1.0, -0.25, 1.75, 0.625, 1.75, -0.4, 3]
    coords = np.concatenate([np.concatenate([np.full((n, 1), b, F32), lattice(rng, n, (0, -24, -8), (56, 24, 8))], axis=1) for b in range(B)])
    coords[0, 1:] = [2.0, 0.0, 0.0]                  # inside box 0
    coords[1, 1:] = [2.0, 0.0, 0.8125]               # above box 0's top (0.75), inside the enlarged box (0.85): ignored
    coords[n, 1:] = [3.0, 1.0, -0.25]                # inside scene 1's box
    feats = rng.standard_normal((B * n, c)).astype(F32)
    out.update(point_coords=coords.astype(F32), point_features=feats, point_gt_boxes=gt, point_cfg=np.array(json.dumps(POINT_CFG)))
    torch.manual_seed(14)
    head = point_mod.PointHeadSimple(num_class=1, input_channels=c, model_cfg=to_attr(copy.deepcopy(POINT_CFG)))
    randomise(head, rng)
    state(head, "point_", out)
    head.train()
    bd = head({'batch_size': B, 'point_features_before_fusion': t(feats.copy()), 'point_features': None,
               'point_coords': t(coords.astype(F32)), 'gt_boxes': t(gt)})
    loss, tb = head.get_loss()
    labels = head.forward_ret_dict['point_cls_labels'].numpy()
    out.update(point_labels=labels, point_loss=np.float32(loss.item()), point_cls_scores=bd['point_cls_scores'].detach().numpy(),
               point_cls_preds=head.forward_ret_dict['point_cls_preds'].detach().numpy())
    print("point: labels", {v: int((labels == v).sum()) for v in (-1, 0, 1)}, "loss", float(loss), tb)
    assert labels[0] == 1 and labels[1] == -1 and labels[n] == 1 and (labels == -1).sum() >= 1


def state_dict_part(root, vsa_mod, point_mod, head_mod):
    model = model_yaml(root, "kitti_models/pv_rcnn.yaml")["MODEL"]
    second = second_settings()
    ds = second["config"]["dataset"]
    pfe_cfg, point_cfg, roi_cfg = model["PFE"], model["POINT_HEAD"], model["ROI_HEAD"]
    n_feat = ds.get("num_point_features", 4)

    def build(num_bev):
        vsa = vsa_mod.VoxelSetAbstraction(to_attr(copy.deepcopy(pfe_cfg)), ds["voxel_size"], np.array(ds["point_cloud_range"]),
                                          num_bev_features=num_bev, num_rawpoint_features=n_feat)
        point = point_mod.PointHeadSimple(num_class=1, input_channels=vsa.num_point_features_before_fusion,
                                          model_cfg=to_attr(copy.deepcopy(point_cfg)))
        head = head_mod.PVRCNNHead(input_channels=vsa.num_point_features, model_cfg=to_attr(copy.deepcopy(roi_cfg)), num_class=1)
        return vsa, point, head

    vsa, point, head = build(model["MAP_TO_BEV"]["NUM_BEV_FEATURES"])
    out = {"VoxelSetAbstraction": shapes(vsa), "PointHeadSimple": shapes(point), "PVRCNNHead": shapes(head)}
    # the whole detector on the reduced grid: SECONDNet's entries with pfe after map_to_bev_module (which has no entries) and
    # point_head after dense_head, the order of the reference's module_topology
    model_cfg = dict(second["config"]["MODEL"], NAME="PVRCNN", PFE=pfe_cfg, POINT_HEAD=point_cfg, ROI_HEAD=roi_cfg)
    vsa, point, head = build(model_cfg["MAP_TO_BEV"]["NUM_BEV_FEATURES"])
    front = [e for e in second["SECONDNet"] if e[0].split(".")[0] in ("vfe", "backbone_3d", "map_to_bev_module")]
    back = [e for e in second["SECONDNet"] if e[0].split(".")[0] in ("backbone_2d", "dense_head")]
    assert len(front) + len(back) == len(second["SECONDNet"])
    out["PVRCNN"] = front + shapes(vsa, "pfe.") + back + shapes(point, "point_head.") + shapes(head, "roi_head.")
    out["config"] = {"MODEL": model_cfg, "dataset": ds, "grid_size": second["config"]["grid_size"],
                     "yaml": {"PFE": pfe_cfg, "POINT_HEAD": point_cfg, "ROI_HEAD": roi_cfg,
                              "NUM_BEV_FEATURES": model["MAP_TO_BEV"]["NUM_BEV_FEATURES"]}}
    write_state_dict("pv_rcnn_state_dict.json", out)


def main():
    root = reference_root()
    pm, vsa_mod, point_mod, head_mod = load_reference(root)
    out = {}
    sa_part(pm, out)
    rng = np.random.default_rng(2026)
    bev_part(vsa_mod, rng, out)
    vsa_part(vsa_mod, rng, out)
    head_part(head_mod, rng, out)
    point_part(point_mod, rng, out)
    path = os.path.join(HERE, "pv_rcnn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    state_dict_part(root, vsa_mod, point_mod, head_mod)


if __name__ == "__main__":
    main()
