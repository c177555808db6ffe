#!/usr/bin/env python
"""Generates tests/golden/pv_rcnn_plusplus.npz and tests/golden/pv_rcnn_plusplus_state_dicts.json from the REFERENCE's own
voxel_set_abstraction.py (sample_points_with_roi, sector_fps, VoxelSetAbstraction with SAMPLE_METHOD SPC and
FILTER_NEIGHBOR_WITH_ROI), pointnet2_stack/pointnet2_modules.py (the three VectorPool classes), pvrcnn_head.py,
point_head_simple.py, spconv_backbone.py, base_bev_backbone.py and center_head.py, imported from where they lie and run on the
CPU.  float32 is the fixture; where a test applies the 4x rule the same run in float64 (reference_loader.precision) lies
next to it as *_f64.

    python tests/golden/make_pv_rcnn_plusplus_golden.py <checkout of the reference>

The `pointnet2_stack_cuda` extension is a stub over the numpy restatements (stack_pool_restatement.py: the two-step three-NN
and vector_pool; stack_sa_restatement.py: farthest-point sampling with the stacked kernel's block of 1024); three_interpolate
and the two gradients are numpy expressions in the arrays' own precision, the gradients added in ascending order (ONE order
the kernels' float atomics can take).  Nothing of the reference is copied; what is committed is data.

pv_rcnn_plusplus.npz
  spc_*    2 scenes of 1 700 and 1 300 points with continuous coordinates, 6 RoIs per scene (two zero rows), 6 sectors (sector 2
           of scene 1 is empty), NUM_KEYPOINTS 64: mask, keys, the (B, 6) segment counts, quotas and keypoints of configuration
           A (spc_rois_a) and of configuration B (spc_rois_b: scene 1 keeps nothing and contributes its first point).
           The inputs are CONSTRUCTED and the generator asserts, in float64 (pv_rcnn_plusplus_restatement.py):
             no point within 1e-4 of its keep threshold, some within 1e-2 on either side;
             no point with two RoIs of different half diagonals at distances within 1e-5 of each other;
             no kept point within 1e-4 rad of a sector boundary;
           and that the float64 statement then gives the reference's mask, keys and quotas.  With these margins the reference
           alone fixes mask, sectors and keypoints (the sampling distances are compared by the numpy restatement in float32
           with the kernels' expression; no tie occurs among continuous coordinates).
  interp_* VectorPoolLocalInterpolateModule(mlp=None) for C in {2, 32} x G in {8, 27}: M = 70 centres in two scenes, scene 1
           has NO support points, some cells of scene 0 have no neighbour.  Kept: the gradient of the support features in
           float32 for the grad_out of pv_rcnn_plusplus_restatement.interp_grad_out, and the error of the float32 rows against
           float64 (the rows themselves would not fit the size limit); the float64 side is pv_rcnn_plusplus_restatement.interp_rows,
           which the generator checks against the reference's own float64 run to 1e-12.  Coordinates on the 1/8 lattice, cell offsets on the 1/4 lattice: distances
           are exact in float32, so the float64 run makes the same neighbour decisions.
  msg_*    one VectorPoolAggregationModuleMSG (two groups: 2x2x2 cells at 1.0, 3x3x3 at 1.5) per LOCAL_AGGREGATION_TYPE in
           train mode: output, gradients of every parameter and of `features`, float32 and float64; and grad_params_err_orders,
           the largest float32 error of the parameter gradients over the same run with the keypoints in 9 orders (see msg_part).
           The generator refuses a
           seed whose float64 run has a ReLU input within 1e-5 of its tensor's largest magnitude of zero (ten float32 roundings;
           among the 50 000 inputs of a module the nearest lies at 1e-6 .. 1e-5, so most seeds are refused).
  vsa_*    VoxelSetAbstraction with SPC keypoints (NUM_KEYPOINTS 48, 16 RoIs per scene, two zero rows), FEATURES_SOURCE bev,
           x_conv2, raw_points, both sources RoI-filtered VectorPool layers, on the 32 x 32 x 16 grid of make_voxel_rcnn_golden:
           keypoints, both feature tensors, gradients of every parameter, of the bev map and of the x_conv2 features, float32 and
           float64; the same margins are asserted for its three filters (on the lattice an exact tie of two distances is decided
           by the index everywhere and is let through), and the ReLU margin.

  point_*  PointHeadSimple over RAGGED keypoints (96 and 61; one point lies only in an enlarged box, one at a place where only the
           other scene has a box): labels of the class-agnostic head and of a three-class head, loss and tb_dict, float32 and
           float64.
  head_*   PVRCNNHead (GRID_SIZE 3, DP_RATIO 0) with a voxel_random_choice VectorPool RoI-grid pool over ragged keypoints (150 and
           110), in train mode on the targets the reference's own assign_targets sampled once (stored as head_target_* and
           handed over as roi_targets_dict): rcnn_cls, rcnn_reg, loss, tb_dict and the gradient of point_features, float32 and
           float64.  RoIs without heading and of sizes 3 and 6: the grid points stay on the lattice.

pv_rcnn_plusplus_state_dicts.json: keys and shapes, in order, of the reference's three VectorPool classes (the msg_* and
interp settings), of VoxelSetAbstraction and PVRCNNHead for waymo_models/pv_rcnn_plusplus.yaml, and of the whole detector of
pv_rcnn_plusplus.yaml and pv_rcnn_plusplus_resnet.yaml in the order of Detector3DTemplate.build_networks (vfe and
map_to_bev_module have no entries), over the spconv stand-in of make_second_state_dict.py; the MODEL block of both yamls (settings only) and the dataset
settings used.
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
import pv_rcnn_plusplus_restatement as pp  # noqa: E402
import stack_pool_restatement as pool  # noqa: E402
import stack_sa_restatement as rs  # noqa: E402
from make_voxel_rcnn_golden import PCR, VOXEL, sparse_level  # noqa: E402
from reference_loader import (MODEL_UTILS, ROI_HEAD, as_np as _np, cpu_torch, extension_stubs, load, model_yaml, np_args,  # noqa: E402
                              precision, randomise, reference_root, shapes, state, stub_numba, write_state_dict)
from pdanet_amd.config import to_attr  # noqa: E402

F32, I32 = np.float32, np.int32
t = torch.from_numpy
WAYMO = {"class_names": ["Vehicle", "Pedestrian", "Cyclist"], "point_cloud_range": [-75.2, -75.2, -2, 75.2, 75.2, 4],
         "voxel_size": [0.1, 0.1, 0.15], "num_point_features": 5}


class Stub(types.ModuleType):
    def __init__(self):
        super().__init__("pointnet2_stack_cuda")

    @staticmethod
    def stack_farthest_point_sampling_wrapper(xyz, temp, xyz_batch_cnt, idx, num_sampled_points):
        start, out = 0, []
        for n, k in zip(_np(xyz_batch_cnt).tolist(), _np(num_sampled_points).tolist()):
            picked = rs.fps(_np(xyz)[start:start + n].astype(F32), k, block=1024)
            assert (picked >= 0).all()
            out.append(picked + start)
            start += n
        _np(idx)[...] = np.concatenate(out)
        return 1

    @staticmethod
    def three_interpolate_wrapper(features, idx, weight, out):
        f, i, w = _np(features), _np(idx).astype(np.int64), _np(weight)
        _np(out)[...] = (w[:, 0:1] * f[i[:, 0]] + w[:, 1:2] * f[i[:, 1]]) + w[:, 2:3] * f[i[:, 2]]

    @staticmethod
    def three_interpolate_grad_wrapper(grad_out, idx, weight, grad_features):
        g, i, w, acc = _np(grad_out), _np(idx).astype(np.int64), _np(weight), _np(grad_features)
        terms = (g[:, None, :] * w[:, :, None]).reshape(-1, g.shape[1])          # row by row, neighbour 0, 1, 2
        np.add.at(acc, i.reshape(-1), terms)

    @staticmethod
    def query_stacked_local_neighbor_idxs_wrapper_stack(*args):
        pool.query_stacked_local_neighbor_idxs(*np_args(args))
        return 0

    @staticmethod
    def query_three_nn_by_stacked_local_idxs_wrapper_stack(*args):
        pool.query_three_nn_by_stacked_local_idxs(*np_args(args))
        return 0

    @staticmethod
    def vector_pool_wrapper(*args):
        return pool.vector_pool(*np_args(args))

    @staticmethod
    def vector_pool_grad_wrapper(grad_new_features, point_cnt_of_grid, grouped_idxs, grad_support_features):
        g, cnt, rows, acc = _np(grad_new_features), _np(point_cnt_of_grid), _np(grouped_idxs).astype(np.int64), _np(grad_support_features)
        n_grids = cnt.shape[1]
        ce = g.shape[1] // n_grids
        k, m, cell = rows[:, 0], rows[:, 1], rows[:, 2]
        norm = np.maximum(cnt[m, cell], 1).astype(g.dtype)
        fold = np.arange(acc.shape[1]) % ce
        np.add.at(acc, k, g.reshape(len(g), n_grids, ce)[m, cell][:, fold] / norm[:, None])
        return 1


def load_reference(root):
    """-> the reference's pointnet2_modules, voxel_set_abstraction, point_head_simple, pvrcnn_head as pcdet_ref.*"""
    cpu_torch()
    stack = "ops.pointnet2.pointnet2_stack."
    load(root, "pcdet_ref", MODEL_UTILS + ROI_HEAD + [stack + "pointnet2_utils", "models.dense_heads.point_head_template"],
         stubs=extension_stubs({stack + "pointnet2_stack_cuda": Stub()}))
    return load(root, "pcdet_ref", [stack + "pointnet2_modules", "models.backbones_3d.pfe.voxel_set_abstraction",
                                    "models.dense_heads.point_head_simple", "models.roi_heads.pvrcnn_head"])


def lattice(rng, n, lo, hi, step=8):
    return np.stack([rng.integers(lo[k] * step, hi[k] * step, n) for k in range(3)], axis=1).astype(F32) / step


# ---- margins ------------------------------------------------------------------------------------------------------------------
def filter_margins(points, counts, rois, radius, num_sectors=0, need_near=False, lattice_input=False):
    """The three conditions of the module docstring over a stacked point set; -> (mask, keys) in float64.  lattice_input: points
    and RoI centres lie on the 1/8 lattice, where squared distances are exact in float32 and an EXACT tie is decided by the index
    on every platform; only ties that are not exact are refused then."""
    masks, keys, start = [], [], 0
    for b, n in enumerate(counts):
        p = points[start:start + n]
        margin, gap = pp.roi_filter(p, rois[b], radius)
        assert np.abs(margin).min() > 1e-4, "a point within 1e-4 of its keep threshold"
        assert (gap[gap > 0] if lattice_input else gap).min(initial=np.inf) > 1e-5, "two RoIs of different half diagonals within 1e-5 of a point's nearest distance"
        if need_near:
            assert ((margin > 0) & (margin < 1e-2)).any() and ((margin < 0) & (margin > -1e-2)).any(), "nobody near the threshold"
        kept = margin < 0
        masks.append(kept)
        if num_sectors:
            pos = pp.sector_position(p, num_sectors)
            assert np.abs(pos[kept] - np.round(pos[kept])).min(initial=1.0) * (np.pi * 2 / num_sectors) > 1e-4, \
                "a kept point within 1e-4 rad of a sector boundary"
            keys.append(pp.sector_keys(b, kept, pos, num_sectors))
        start += n
    return np.concatenate(masks), (np.concatenate(keys) if num_sectors else None)


def relu_margin(module):
    """Hooks every ReLU of `module`; the returned list gets min |input| / max |input| of each call."""
    seen = []
    for m in module.modules():
        if isinstance(m, torch.nn.ReLU):
            m.register_forward_hook(lambda mod, inp, out: seen.append(float(inp[0].abs().min() / inp[0].abs().max())))
    return seen


# ---- spc ------------------------------------------------------------------------------------------------------------------
SPC = dict(counts=[1700, 1300], radius=1.6, sectors=6, keypoints=64)


def spc_points(rng, n, rois, radius, empty_sector=None, far_from_origin=False):
    """n continuous points around the RoIs that meet the margins, some of them CONSTRUCTED next to their keep threshold."""
    out = []
    while sum(len(o) for o in out) < n:
        p = rng.uniform([-12, -12, -2], [12, 12, 2], (4 * n, 3))
        if not out:                                                  # on both sides of the threshold of RoI 0 and of a zero row
            for r in (rois[0], rois[-1]):
                half = np.sqrt(((r[3:6] / 2) ** 2).sum())
                u = rng.standard_normal((24, 3))
                u /= np.linalg.norm(u, axis=1, keepdims=True)
                p[:24] = r[:3] + u * (half + radius + rng.choice([-1, 1], (24, 1)) * rng.uniform(2e-3, 8e-3, (24, 1)))
                p = np.roll(p, 24, axis=0)
        p = p.astype(F32)
        margin, gap = pp.roi_filter(p, rois, radius)
        pos = pp.sector_position(p, SPC['sectors'])
        ok = (np.abs(margin) > 2e-4) & (gap > 2e-5) & (np.abs(pos - np.round(pos)) * (np.pi / 3) > 2e-4)
        if empty_sector is not None:
            ok &= np.floor(pos) != empty_sector
        if far_from_origin:
            ok &= np.linalg.norm(p[:, :2], axis=1) > 4.0
        out.append(p[ok])
    p = np.concatenate(out)[:n]
    return p[rng.permutation(n)]


def spc_part(vsa_mod, rng, out):
    B, counts, S, K, radius = 2, SPC['counts'], SPC['sectors'], SPC['keypoints'], SPC['radius']
    rois = np.zeros((B, 6, 7), F32)
    angle = np.deg2rad(np.array([[-150.0, -50.0, 50.0, 150.0], [-160.0, -100.0, 40.0, 130.0]]) + rng.uniform(-5, 5, (B, 4)))
    rois[:, :4, 0], rois[:, :4, 1] = 6.0 * np.cos(angle), 6.0 * np.sin(angle)     # around the origin, where the zero rows sit
    rois[:, :4, 2] = rng.uniform(-1, 1, (B, 4))
    rois[:, :4, 3:6] = rng.uniform([3.0, 1.5, 1.4], [5.0, 2.2, 2.0], (B, 4, 3))
    rois[:, :4, 6] = rng.uniform(-3, 3, (B, 4))
    rois[0] = rois[0, [0, 4, 1, 2, 5, 3]]                                 # the zero rows in the middle and at the end
    rois_b = rois.copy()
    rois_b[1, :, 0:2] = np.where(rois_b[1, :, 3:4] > 0, 500.0, 0.0)       # configuration B: scene 1's boxes far away
    pts = [spc_points(rng, counts[0], rois[0], radius), spc_points(rng, counts[1], rois[1], radius, empty_sector=2, far_from_origin=True)]
    points = np.concatenate(pts).astype(F32)
    out.update(spc_points=points, spc_counts=np.array(counts, I32), spc_rois_a=rois, spc_rois_b=rois_b,
               spc_settings=np.array([radius, S, K], np.float64))
    cfg = to_attr({'POINT_SOURCE': 'raw_points', 'SAMPLE_METHOD': 'SPC', 'NUM_KEYPOINTS': K,
                   'SPC_SAMPLING': {'NUM_SECTORS': S, 'SAMPLE_RADIUS_WITH_ROI': radius}})
    obj = vsa_mod.VoxelSetAbstraction.__new__(vsa_mod.VoxelSetAbstraction)
    obj.__dict__['model_cfg'] = cfg
    batch_pts = np.concatenate([np.repeat(np.arange(B), counts)[:, None].astype(F32), points], axis=1)
    for tag, r in (("a", rois), ("b", rois_b)):
        mask64, keys64 = filter_margins(points, counts, r, radius, S, need_near=(tag == "a"))
        masks, keys, seg, quota, start = [], [], [], [], 0
        for b, n in enumerate(counts):
            p = t(points[start:start + n])
            _, m = vsa_mod.sample_points_with_roi(rois=t(r[b]), points=p, sample_radius_with_roi=radius, num_max_points_of_part=700)
            ang = torch.atan2(p[:, 1], p[:, 0]) + np.pi                   # the reference's own float32 expressions (sector_fps)
            sec = (ang / (np.pi * 2 / S)).floor().clamp(min=0, max=S).long()
            masks.append(m.numpy())
            keys.append((b * (S + 1) + torch.where(m, sec, torch.full_like(sec, S))).numpy())
            cnt = [int((m & (sec == k)).sum()) for k in range(S)]
            seg.append(cnt)
            quota.append(pp.quotas(cnt, int(m.sum()), K) if m.any() else [0] * S)
            start += n
        mask, keys = np.concatenate(masks), np.concatenate(keys)
        assert np.array_equal(mask, mask64) and np.array_equal(keys, keys64), "float64 decides otherwise"
        kp = vsa_mod.VoxelSetAbstraction.get_sampled_points(obj, {'batch_size': B, 'points': t(batch_pts), 'rois': t(r)}).numpy()
        per_scene = [int((kp[:, 0] == b).sum()) for b in range(B)]
        assert per_scene == [max(sum(q), 1) for q in quota], (per_scene, quota)
        print("spc", tag, "kept", [int(m.sum()) for m in masks], "segments", seg, "quotas", quota, "keypoints", per_scene)
        out.update({"spc_mask_" + tag: mask.astype(np.uint8), "spc_keys_" + tag: keys.astype(I32), "spc_seg_" + tag: np.array(seg, np.int64),
                    "spc_quota_" + tag: np.array(quota, np.int64), "spc_keypoints_" + tag: kp})
        if tag == "a":
            assert all(sum(q) != K for q in quota) and min(seg[0]) > 0 and [c > 0 for c in seg[1]] == [True, True, False, True, True, True]
            assert any(q * sum(s) != c * K for s, qs in zip(seg, quota) for c, q in zip(s, qs) if c), "no quota rounds up"
        else:
            assert masks[1].sum() == 0 and per_scene[1] == 1 and np.array_equal(kp[-1, 1:], points[counts[0]])


# ---- interpolation rows -----------------------------------------------------------------------------------------------------
def interp_part(pm, rng, out):
    xyz_cnt, new_cnt = np.array([150, 0], I32), np.array([40, 30], I32)
    xyz = lattice(rng, 150, (-3, -3, -2), (3, 3, 2))
    new_xyz = lattice(rng, 70, (-3, -3, -2), (3, 3, 2))
    new_xyz[:3] += 30                                                     # no neighbour at all
    out.update(interp_xyz=xyz, interp_xyz_cnt=xyz_cnt, interp_new_xyz=new_xyz, interp_new_cnt=new_cnt)
    for c in (2, 32):
        feat = rng.standard_normal((150, c)).astype(F32)
        out["interp_feat_c%d" % c] = feat
        for n_side, dist in ((2, 0.5), (3, 0.75)):
            g = n_side ** 3
            tag = "interp_c%d_g%d_" % (c, g)
            grad_out = pp.interp_grad_out(70 * g, c + 9)
            mod = pm.VectorPoolLocalInterpolateModule(mlp=None, num_voxels=[n_side] * 3, max_neighbour_distance=dist, nsample=-1,
                                                      neighbor_type=0, neighbour_distance_multiplier=2.0)
            centers = pm.VectorPoolAggregationModule.get_dense_voxels_by_center(t(new_xyz), dist, [n_side] * 3)
            got = {}
            for dtype, suffix in ((torch.float32, ""), (torch.float64, "_f64")):
                with precision(dtype):
                    f = t(feat).to(dtype).requires_grad_(True)
                    rows = mod(t(xyz).to(dtype), f, t(xyz_cnt), t(new_xyz).to(dtype), centers.to(dtype), t(new_cnt))
                    (rows * t(grad_out).to(dtype)).sum().backward()
                got["rows" + suffix], got["grad" + suffix] = rows.detach().numpy(), f.grad.numpy()
            # the float64 restatement over the same neighbours agrees with the reference's float64 run
            with torch.no_grad():
                _, idx, _ = pm.pointnet2_utils.three_nn_for_vector_pool_by_two_step(
                    t(xyz), t(xyz_cnt), t(new_xyz), centers, t(new_cnt), dist, -1, 0, 1000, g, 2.0)
            f = t(feat).double().requires_grad_(True)
            mine = pp.interp_rows(t(xyz), f, centers, idx)
            (mine * t(grad_out).double().view(70, -1)).sum().backward()
            assert np.abs(mine.detach().numpy().reshape(-1, c + 9) - got["rows_f64"]).max() < 1e-12
            assert np.abs(f.grad.numpy() - got["grad_f64"]).max() < 1e-10
            empty = (idx.numpy()[..., 0] < 0)
            assert empty[:40].any() and not empty[:40].all() and empty[40:].all()
            # the float64 side is the restatement's (checked above); of the float32 rows only their error is kept: the file's size
            out[tag + "rows_err"] = np.float64(np.abs(got["rows"] - got["rows_f64"]).max() / np.abs(got["rows_f64"]).max())
            out[tag + "grad"], out[tag + "dist"] = got["grad"], np.float64(dist)
            print(tag, "cells without neighbour in scene 0:", int(empty[:40].sum()), "of", empty[:40].size,
                  "float32 error of the rows %.2e" % out[tag + "rows_err"])


# ---- one VectorPoolAggregationModuleMSG per aggregation type ---------------------------------------------------------------------
def msg_cfg(kind, reduced, nsample=-1, width=16):
    return {'NAME': 'VectorPoolAggregationModuleMSG', 'NUM_GROUPS': 2, 'LOCAL_AGGREGATION_TYPE': kind, 'NUM_REDUCED_CHANNELS': reduced,
            'NUM_CHANNELS_OF_LOCAL_AGGREGATION': 4, 'MSG_POST_MLPS': [width],
            'GROUP_CFG_0': {'NUM_LOCAL_VOXEL': [2, 2, 2], 'MAX_NEIGHBOR_DISTANCE': 1.0, 'NEIGHBOR_NSAMPLE': nsample, 'POST_MLPS': [8, 8]},
            'GROUP_CFG_1': {'NUM_LOCAL_VOXEL': [3, 3, 3], 'MAX_NEIGHBOR_DISTANCE': 1.5, 'NEIGHBOR_NSAMPLE': nsample, 'POST_MLPS': [8, 8]}}


MSG_KINDS = (('local_interpolation', -1), ('voxel_avg_pool', -1), ('voxel_random_choice', 8))
ORDERS = 8


def run_both(make, forward, what, keep_param_grads=True):
    """make() -> a fresh float32 module (the same every time); forward(module, dtype) -> (outputs dict, loss, extra tensors that
    require grad).  Runs float32 and float64 in train mode -> {name + suffix: array}, or None when a ReLU input of the
    float64 run lies within 1e-5 of its tensor's largest magnitude of zero."""
    res = {}
    for dtype, suffix in ((torch.float32, ""), (torch.float64, "_f64")):
        mod = make().to(dtype).train()
        seen = relu_margin(mod)
        with precision(dtype):
            outputs, loss, extra = forward(mod, dtype)
            loss.backward()
        if dtype == torch.float64 and min(seen) <= 1e-5:
            print(what, "refused: a ReLU input at %.1e of the largest" % min(seen))
            return None
        for k, v in outputs.items():
            res[k + suffix] = v.detach().numpy()
        for k, v in extra.items():
            res["grad_" + k + suffix] = v.grad.numpy()
        for k, p in mod.named_parameters():
            assert p.grad is not None, k
            if keep_param_grads:
                res["grad." + k + suffix] = p.grad.numpy().copy()
    return res


def msg_part(pm, out):
    for kind, nsample in MSG_KINDS:
        cfg = msg_cfg(kind, 4, nsample)
        for seed in range(200):
            rng = np.random.default_rng(8100 + seed)
            xyz_cnt, new_cnt = np.array([170, 130], I32), np.array([40, 30], I32)
            xyz = lattice(rng, 300, (-3, -3, -2), (3, 3, 2))
            new_xyz = lattice(rng, 70, (-3, -3, -2), (3, 3, 2))
            new_xyz[-2:] += 30
            feat = rng.standard_normal((300, 8)).astype(F32)
            grad_out = rng.standard_normal((70, 16)).astype(F32)

            def make():
                torch.manual_seed(31)
                mod = pm.VectorPoolAggregationModuleMSG(input_channels=8, config=to_attr(copy.deepcopy(cfg)))
                randomise(mod, np.random.default_rng(8100 + seed))
                return mod

            def forward(mod, dtype):
                f = t(feat).to(dtype).requires_grad_(True)
                _, res = mod(xyz=t(xyz).to(dtype), xyz_batch_cnt=t(xyz_cnt), new_xyz=t(new_xyz).to(dtype), new_xyz_batch_cnt=t(new_cnt),
                             features=f)
                return {"out": res}, (res * t(grad_out).to(dtype)).sum(), {"features": f}

            res = run_both(make, forward, "msg " + kind)
            if res is not None:
                break
        else:
            raise SystemExit("msg_part: no seed meets the ReLU margin")
        tag = "msg_%s_" % kind
        out.update({tag + k: v for k, v in res.items()})
        out.update({tag + "xyz": xyz, tag + "xyz_cnt": xyz_cnt, tag + "new_xyz": new_xyz, tag + "new_cnt": new_cnt, tag + "features": feat,
                    tag + "grad_out": grad_out, tag + "cfg": np.array(json.dumps(cfg))})
        state(make(), tag, out)
        # the yardstick of the parameter gradients: they are float32 sums over the keypoints, and ONE order of the keypoints gives
        # one sample of that sum's rounding error.  The same float32 run is repeated with the keypoints of each scene (and the rows
        # of grad_out with them) in ORDERS other orders, which changes no gradient mathematically; the largest error among all
        # orders is kept next to the single run's.
        truth = {k[5:-4]: v for k, v in res.items() if k.startswith("grad.") and k.endswith("_f64")}
        scale = max(np.abs(v).max() for v in truth.values())
        errs = [max(np.abs(res["grad." + k] - v).max() for k, v in truth.items()) / scale]
        for order in range(ORDERS):
            prng = np.random.default_rng(600 + order)
            perm = np.concatenate([prng.permutation(int(new_cnt[0])), int(new_cnt[0]) + prng.permutation(int(new_cnt[1]))])
            mod = make().train()
            _, got = mod(xyz=t(xyz), xyz_batch_cnt=t(xyz_cnt), new_xyz=t(np.ascontiguousarray(new_xyz[perm])), new_xyz_batch_cnt=t(new_cnt),
                         features=t(feat.copy()))
            (got * t(np.ascontiguousarray(grad_out[perm]))).sum().backward()
            errs.append(max(np.abs(p.grad.numpy() - truth[k]).max() for k, p in mod.named_parameters()) / scale)
        out[tag + "grad_params_err_orders"] = np.float64(max(errs))
        print(tag, "seed", seed, "float32 error of the output %.2e" % np.abs(res["out"] - res["out_f64"]).max(),
              "of the parameter gradients: one order %.2e, the largest of %d orders %.2e" % (errs[0], ORDERS + 1, max(errs)))


# ---- the SPC VoxelSetAbstraction -------------------------------------------------------------------------------------------------
def vsa_cfg():
    raw = dict(msg_cfg('local_interpolation', 1, width=16), FILTER_NEIGHBOR_WITH_ROI=True, RADIUS_OF_NEIGHBOR_WITH_ROI=2.4)
    conv = dict(msg_cfg('local_interpolation', 8, width=16), FILTER_NEIGHBOR_WITH_ROI=True, RADIUS_OF_NEIGHBOR_WITH_ROI=3.1,
                DOWNSAMPLE_FACTOR=2, INPUT_CHANNELS=16)
    return {'NAME': 'VoxelSetAbstraction', 'POINT_SOURCE': 'raw_points', 'NUM_KEYPOINTS': 48, 'NUM_OUTPUT_FEATURES': 32,
            'SAMPLE_METHOD': 'SPC', 'SPC_SAMPLING': {'NUM_SECTORS': 6, 'SAMPLE_RADIUS_WITH_ROI': 1.6},
            'FEATURES_SOURCE': ['bev', 'x_conv2', 'raw_points'], 'SA_LAYER': {'raw_points': raw, 'x_conv2': conv}}


VSA_BEV = (16, 8, 8)


def vsa_part(vsa_mod, cu, out):
    B, counts, n_roi = 2, [260, 200], 16
    cfg = vsa_cfg()
    for seed in range(300):
        rng = np.random.default_rng(9300 + seed)
        pts = []
        for b, n in enumerate(counts):
            xyz = np.unique(lattice(rng, n + 60, PCR[:3], PCR[3:]), axis=0)
            xyz = xyz[xyz[:, 1] != 0]                                     # y = 0 is a sector boundary
            xyz = xyz[rng.permutation(len(xyz))[:n]]
            assert len(xyz) == n
            pts.append(np.concatenate([np.full((n, 1), b), xyz, rng.random((n, 1))], axis=1))
        points = np.concatenate(pts).astype(F32)
        ind, feat, shape = sparse_level(rng, 2, [300, 200], 16)
        rois = np.zeros((B, n_roi, 7), F32)
        rois[:, :14, 0:3] = lattice(rng, B * 14, PCR[:3], PCR[3:]).reshape(B, 14, 3)
        rois[:, :14, 3:6] = rng.integers(1, 5, (B, 14, 3)) * 0.5
        rois[:, :14, 6] = rng.uniform(-3, 3, (B, 14))
        conv_xyz = cu.get_voxel_centers(t(ind[:, 1:4]), 2, VOXEL, PCR).numpy()
        try:
            filter_margins(points[:, 1:4], counts, rois, 1.6, 6, lattice_input=True)
            filter_margins(points[:, 1:4], counts, rois, 2.4, lattice_input=True)
            filter_margins(conv_xyz, [300, 200], rois, 3.1, lattice_input=True)
        except AssertionError as e:
            print("vsa seed", seed, "refused:", e)
            continue
        bev = rng.standard_normal((B,) + VSA_BEV).astype(F32)

        def make():
            torch.manual_seed(17)
            mod = vsa_mod.VoxelSetAbstraction(to_attr(copy.deepcopy(cfg)), VOXEL, PCR, num_bev_features=VSA_BEV[0], num_rawpoint_features=4)
            randomise(mod, np.random.default_rng(9300 + seed))
            return mod

        grad_seed = np.random.default_rng(77)
        g_before, g_after = grad_seed.standard_normal((4096, 16 + 16 + 16)).astype(F32), grad_seed.standard_normal((4096, 32)).astype(F32)

        def forward(mod, dtype):
            f, m = t(feat).to(dtype).requires_grad_(True), t(bev).to(dtype).requires_grad_(True)
            bd = mod({'batch_size': B, 'points': t(points).to(dtype), 'rois': t(rois).to(dtype), 'spatial_features': m,
                      'spatial_features_stride': 4,
                      'multi_scale_3d_features': {'x_conv2': types.SimpleNamespace(indices=t(ind), features=f)}})
            n = bd['point_features'].shape[0]
            loss = (bd['point_features'] * t(g_after[:n]).to(dtype)).sum() + (bd['point_features_before_fusion'] * t(g_before[:n]).to(dtype)).sum()
            return ({"before_fusion": bd['point_features_before_fusion'], "point_features": bd['point_features'],
                     "point_coords": bd['point_coords']}, loss, {"x_conv2": f, "bev": m})

        res = run_both(make, forward, "vsa")
        if res is not None:
            break
    else:
        raise SystemExit("vsa_part: no seed meets the margins")
    assert np.array_equal(res["point_coords"], res["point_coords_f64"].astype(F32))
    n = len(res["point_coords"])
    out.update({"vsa_" + k: v for k, v in res.items()})
    out.update(vsa_points=points, vsa_rois=rois, vsa_bev=bev, vsa_x_conv2_indices=ind, vsa_x_conv2_features=feat,
               vsa_x_conv2_spatial_shape=np.array(shape, I32), vsa_cfg=np.array(json.dumps(cfg)), vsa_grad_before=g_before[:n],
               vsa_grad_after=g_after[:n])
    state(make(), "vsa_", out)
    print("vsa: seed", seed, "keypoints per scene", [int((res["point_coords"][:, 0] == b).sum()) for b in range(B)],
          "float32 error of point_features %.2e" % np.abs(res["point_features"] - res["point_features_f64"]).max())


# ---- the point head and the RoI head on ragged keypoints ---------------------------------------------------------------------------
POINT_CFG = {'NAME': 'PointHeadSimple', 'CLS_FC': [32, 32], 'CLASS_AGNOSTIC': True, 'USE_POINT_FEATURES_BEFORE_FUSION': True,
             'TARGET_CONFIG': {'GT_EXTRA_WIDTH': [0.2, 0.2, 0.2]},
             'LOSS_CONFIG': {'LOSS_REG': 'smooth-l1', 'LOSS_WEIGHTS': {'point_cls_weight': 1.0}}}


def point_part(point_mod, out):
    counts, c = [96, 61], 24                                    # ragged, as SPC leaves the keypoints
    gt = np.zeros((2, 3, 8), F32)
    gt[0, 0] = [2.0, 0.0, 0.0, 3.0, 1.5, 1.5, 0.3, 1]
    gt[0, 1] = [5.5, -2.0, 0.25, 1.0, 0.75, 1.75, 1.2, 2]
    gt[1, 0] = [3.0, 1.0, -0.25, 1.75, 0.625, 1.75, -0.4, 3]
    gt[1, 1] = [6.0, -1.0, 0.5, 2.0, 2.0, 2.0, 0.0, 2]
    for seed in range(200):
        rng = np.random.default_rng(9700 + seed)
        coords = np.concatenate([np.concatenate([np.full((n, 1), b, F32), lattice(rng, n, (0, -3, -1), (7, 3, 1))], axis=1)
                                 for b, n in enumerate(counts)]).astype(F32)
        coords[0, 1:] = [2.0, 0.0, 0.0]                         # inside box 0
        coords[1, 1:] = [2.0, 0.0, 0.8125]                      # above box 0's top (0.75), inside the enlarged box (0.85): ignored
        coords[counts[0], 1:] = [3.0, 1.0, -0.25]               # inside scene 1's first box
        coords[counts[0] + 1, 1:] = [2.0, 0.0, 0.0]             # scene 1 has no box there: a scene mix-up would label it
        feats = rng.standard_normal((len(coords), c)).astype(F32)

        def make():
            torch.manual_seed(14)
            head = point_mod.PointHeadSimple(num_class=1, input_channels=c, model_cfg=to_attr(copy.deepcopy(POINT_CFG)))
            randomise(head, np.random.default_rng(9700 + seed))
            return head

        labels = {}

        def forward(head, dtype):
            head({'batch_size': 2, 'point_features_before_fusion': t(feats).to(dtype), 'point_features': None, 'point_coords': t(coords).to(dtype),
                  'gt_boxes': t(gt).to(dtype)})
            loss, tb = head.get_loss()
            labels[dtype] = head.forward_ret_dict['point_cls_labels'].numpy().copy()
            return {"loss": loss, "tb_point_loss_cls": torch.tensor(tb['point_loss_cls'], dtype=dtype)}, loss, {}

        res = run_both(make, forward, "point", keep_param_grads=False)
        if res is not None:
            break
    else:
        raise SystemExit("point_part: no seed meets the ReLU margin")
    assert np.array_equal(labels[torch.float32], labels[torch.float64])
    lab = labels[torch.float32]
    assert lab[0] == 1 and lab[1] == -1 and lab[counts[0]] == 1 and lab[counts[0] + 1] == 0 and (lab == -1).sum() >= 1
    # the labels of a three-class head over the same points: the class of the box
    head3 = point_mod.PointHeadSimple(num_class=3, input_channels=c, model_cfg=to_attr(dict(copy.deepcopy(POINT_CFG), CLASS_AGNOSTIC=False)))
    lab3 = head3.assign_targets({'point_coords': t(coords), 'gt_boxes': t(gt)})['point_cls_labels'].numpy()
    assert set(np.unique(lab3)) >= {-1, 0, 1, 3} and np.array_equal(lab3 > 0, lab > 0)
    out.update({"point_" + k: v for k, v in res.items()})
    out.update(point_coords=coords, point_features=feats, point_gt_boxes=gt, point_labels=lab, point_labels_3=lab3,
               point_cfg=np.array(json.dumps(POINT_CFG)))
    state(make(), "point_", out)
    print("point: seed", seed, "labels", {v: int((lab == v).sum()) for v in (-1, 0, 1)}, "three classes", {int(v): int((lab3 == v).sum()) for v in np.unique(lab3)},
          "loss %.6f, float32 error %.2e" % (res["loss_f64"], abs(res["loss"] - res["loss_f64"]) / abs(res["loss_f64"])))


def head_cfg():
    pool = dict(msg_cfg('voxel_random_choice', 4, 8, width=16), GRID_SIZE=3)
    return {'NAME': 'PVRCNNHead', 'CLASS_AGNOSTIC': True, 'SHARED_FC': [32, 32], 'CLS_FC': [32, 32], 'REG_FC': [32, 32], 'DP_RATIO': 0.0,
            'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000, 'NMS_POST_MAXSIZE': 512,
                                     'NMS_THRESH': 0.8},
                           'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 1024, 'NMS_POST_MAXSIZE': 100,
                                    'NMS_THRESH': 0.7}},
            'ROI_GRID_POOL': pool,
            'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 8, 'FG_RATIO': 0.5, 'SAMPLE_ROI_BY_EACH_CLASS': True,
                              'CLS_SCORE_TYPE': 'roi_iou', 'CLS_FG_THRESH': 0.75, 'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1,
                              'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55},
            'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                            'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,
                                             'code_weights': [1.0] * 7}}}


TARGET_KEYS = ('rois', 'gt_of_rois', 'gt_of_rois_src', 'gt_iou_of_rois', 'roi_scores', 'roi_labels', 'reg_valid_mask', 'rcnn_cls_labels')


def head_part(head_mod, out):
    """The reference's PVRCNNHead with a VectorPool RoI-grid pool over ragged keypoints: the targets the reference samples once
    (float32, seeded) are stored and handed to both runs as roi_targets_dict, which the head takes as they are."""
    B, n_roi, per_scene, c_in = 2, 12, [150, 110], 8
    cfg = head_cfg()
    for seed in range(200):
        rng = np.random.default_rng(9900 + seed)
        coords = np.concatenate([np.concatenate([np.full((n, 1), b, F32), lattice(rng, n, (0, -4, -2), (8, 4, 2))], axis=1)
                                 for b, n in enumerate(per_scene)]).astype(F32)
        feats = rng.standard_normal((len(coords), c_in)).astype(F32)
        scores = rng.random(len(coords)).astype(F32)
        rois = np.zeros((B, n_roi, 7), F32)
        rois[..., 0:3] = lattice(rng, B * n_roi, (1, -3, -1), (7, 3, 1)).reshape(B, n_roi, 3)
        rois[..., 3:6] = rng.integers(1, 3, (B, n_roi, 3)) * 3           # sizes 3 or 6 and no heading: the grid points stay on the lattice
        rois[1, -1] = 0                                                  # a zero-padded RoI row
        gt = np.zeros((B, 4, 8), F32)
        for b in range(B):                                               # boxes that overlap the first RoIs well, partly, hardly
            for k, shift in enumerate((0.125, 0.5, 1.0, 2.0)):
                gt[b, k, :7] = rois[b, k]
                gt[b, k, 0] += shift
                gt[b, k, 7] = 1 + k % 3
        torch.manual_seed(99 + seed)
        np.random.seed(99 + seed)
        sampler = head_mod.PVRCNNHead(input_channels=c_in, model_cfg=to_attr(copy.deepcopy(cfg)), num_class=1)
        targets = sampler.assign_targets({'batch_size': B, 'rois': t(rois.copy()), 'roi_scores': t(rng.random((B, n_roi)).astype(F32)),
                                          'roi_labels': torch.ones(B, n_roi, dtype=torch.long), 'gt_boxes': t(gt)})
        targets = {k: targets[k].numpy().copy() for k in TARGET_KEYS}
        if not ((targets['rcnn_cls_labels'] > 0.5).any() and (targets['rcnn_cls_labels'] == 0).any() and targets['reg_valid_mask'].any()):
            continue

        def make():
            torch.manual_seed(12)
            head = head_mod.PVRCNNHead(input_channels=c_in, model_cfg=to_attr(copy.deepcopy(cfg)), num_class=1)
            randomise(head, np.random.default_rng(9900 + seed))
            with torch.no_grad():                           # the reference's std 0.001 would leave the predictions at zero
                head.cls_layers[-1].weight.normal_(0, 0.3, generator=torch.Generator().manual_seed(5))
                head.reg_layers[-1].weight.normal_(0, 0.1, generator=torch.Generator().manual_seed(6))
            return head

        def forward(head, dtype):
            cast = lambda a: t(a.copy()).to(dtype) if a.dtype == F32 else t(a.copy())
            tgt = {k: cast(v) for k, v in targets.items()}
            f = t(feats).to(dtype).requires_grad_(True)
            head({'batch_size': B, 'rois': tgt['rois'], 'roi_labels': tgt['roi_labels'], 'roi_targets_dict': tgt, 'point_coords': t(coords).to(dtype),
                  'point_features': f, 'point_cls_scores': t(scores).to(dtype)})
            loss, tb = head.get_loss()
            outs = {"tb_" + k: torch.tensor(v, dtype=dtype) for k, v in tb.items()}
            outs.update(loss=loss, rcnn_cls=head.forward_ret_dict['rcnn_cls'], rcnn_reg=head.forward_ret_dict['rcnn_reg'])
            return outs, loss, {"point_features": f}

        res = run_both(make, forward, "head", keep_param_grads=False)
        if res is not None:
            break
    else:
        raise SystemExit("head_part: no seed meets the margins")
    out.update({"head_" + k: v for k, v in res.items()})
    out.update({"head_target_" + k: v for k, v in targets.items()})
    out.update(head_point_coords=coords, head_point_features=feats, head_point_cls_scores=scores, head_cfg=np.array(json.dumps(cfg)),
               head_c_in=np.int32(c_in))
    state(make(), "head_", out)
    print("head: seed", seed, "labels", np.round(targets['rcnn_cls_labels'], 2).tolist(), "valid", int(targets['reg_valid_mask'].sum()),
          {k: float(v) for k, v in res.items() if k.startswith("tb_") and k.endswith("_f64")},
          "float32 error of the loss %.2e" % (abs(res["loss"] - res["loss_f64"]) / abs(res["loss_f64"])))


# ---- state dicts -------------------------------------------------------------------------------------------------------------
def state_dict_part(root, pm, vsa_mod, point_mod, head_mod):
    from make_second_state_dict import _spconv_stand_in
    _spconv_stand_in()
    stub_numba()
    load(root, "pcdet_ref", ["utils.spconv_utils"])
    b3d, b2d, center = load(root, "pcdet_ref", ["models.model_utils.centernet_utils", "models.backbones_3d.spconv_backbone",
                                                "models.backbones_2d.base_bev_backbone", "models.dense_heads.center_head"])[1:]
    out = {"dataset": WAYMO, "config": {}}
    out["VectorPoolLocalInterpolateModule"] = shapes(pm.VectorPoolLocalInterpolateModule(
        mlp=[8, 16, 16], num_voxels=[3, 3, 3], max_neighbour_distance=1.0, nsample=-1, neighbor_type=0))
    out["VectorPoolAggregationModule"] = shapes(pm.VectorPoolAggregationModule(
        input_channels=8, num_reduced_channels=4, num_channels_of_local_aggregation=4, post_mlps=(8, 8), max_neighbor_distance=1.0))
    out["VectorPoolAggregationModuleMSG"] = shapes(pm.VectorPoolAggregationModuleMSG(
        input_channels=8, config=to_attr(msg_cfg('voxel_random_choice', 4, 8))))
    pcr, vs = np.array(WAYMO["point_cloud_range"], np.float64), WAYMO["voxel_size"]
    grid = np.round((pcr[3:] - pcr[:3]) / np.array(vs)).astype(np.int64)
    for name in ("pv_rcnn_plusplus", "pv_rcnn_plusplus_resnet"):
        out["config"][name] = model_yaml(root, "waymo_models/%s.yaml" % name)["MODEL"]
        cfg = to_attr(copy.deepcopy(out["config"][name]))
        backbone_3d = getattr(b3d, cfg.BACKBONE_3D.NAME)(cfg.BACKBONE_3D, WAYMO["num_point_features"], grid)
        pfe = vsa_mod.VoxelSetAbstraction(copy.deepcopy(cfg.PFE), vs, pcr, num_bev_features=cfg.MAP_TO_BEV.NUM_BEV_FEATURES,
                                          num_rawpoint_features=WAYMO["num_point_features"])
        bev = b2d.BaseBEVBackbone(cfg.BACKBONE_2D, input_channels=cfg.MAP_TO_BEV.NUM_BEV_FEATURES)
        dense = center.CenterHead(model_cfg=cfg.DENSE_HEAD, input_channels=bev.num_bev_features, num_class=3,
                                  class_names=WAYMO["class_names"], grid_size=grid, point_cloud_range=pcr, voxel_size=vs,
                                  predict_boxes_when_training=True)
        point = point_mod.PointHeadSimple(num_class=1, input_channels=pfe.num_point_features_before_fusion, model_cfg=copy.deepcopy(cfg.POINT_HEAD))
        head = head_mod.PVRCNNHead(input_channels=pfe.num_point_features, model_cfg=copy.deepcopy(cfg.ROI_HEAD), num_class=1)
        out[name] = (shapes(backbone_3d, "backbone_3d.") + shapes(pfe, "pfe.") + shapes(bev, "backbone_2d.") + shapes(dense, "dense_head.")
                     + shapes(point, "point_head.") + shapes(head, "roi_head."))
        if name == "pv_rcnn_plusplus":
            out["VoxelSetAbstraction"], out["PVRCNNHead"] = shapes(pfe), shapes(head)
    write_state_dict("pv_rcnn_plusplus_state_dicts.json", out)


def main():
    root = reference_root()
    pm, vsa_mod, point_mod, head_mod = load_reference(root)
    cu = sys.modules["pcdet_ref.utils.common_utils"]
    out = {}
    spc_part(vsa_mod, np.random.default_rng(4242), out)
    interp_part(pm, np.random.default_rng(4343), out)
    msg_part(pm, out)
    vsa_part(vsa_mod, cu, out)
    point_part(point_mod, out)
    head_part(head_mod, out)
    path = os.path.join(HERE, "pv_rcnn_plusplus.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)
    state_dict_part(root, pm, vsa_mod, point_mod, head_mod)


if __name__ == "__main__":
    main()
