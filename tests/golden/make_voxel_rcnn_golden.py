#!/usr/bin/env python
"""Generates tests/golden/voxel_rcnn.npz and tests/golden/voxel_rcnn_state_dict.json from the REFERENCE's own
voxel_pool_modules.py, voxel_query_utils.py and voxelrcnn_head.py, imported from where they lie and run on the CPU.

    python tests/golden/make_voxel_rcnn_golden.py <checkout of the reference>

The `pointnet2_stack_cuda` extension is a stub: voxel_query_wrapper is stack_pool_restatement.voxel_query, the two grouping
entry points are numpy gathers.  The loading and the CPU patches are reference_loader.py's.  Nothing of the reference is
copied; what is committed is data.

voxel_rcnn.npz
  pool_*   NeighborVoxelSAModuleMSG with two scales (C = 32 and 64, nsample 16 and 4): inputs, every parameter and buffer,
           the train-mode output, the gradients of sum(out * grad_out) for every parameter and for `features`, the running
           statistics after that step, and the eval-mode output.
  head_*   VoxelRCNNHead (GRID_SIZE 4, DP_RATIO 0, two sources with C = 32 and 64, narrow fc stacks) on given rois: parameters and buffers, roi_grid_pool's and
           the two predictions' values in train and eval mode, and eval's decoded batch_cls_preds / batch_box_preds.
Voxel centres, RoI centres and RoI grid points lie on the 1/8 lattice (voxel size 1/4, RoI sizes whole numbers, heading 0),
so every squared distance is exact in float32 and the query does not depend on the contraction mode.

voxel_rcnn_state_dict.json: keys and shapes, in order, of the reference's VoxelRCNNHead for kitti_models/voxel_rcnn_car.yaml
(backbone_channels of VoxelBackBone8x), and of the whole VoxelRCNN on the settings of second_state_dict.json (its 16 x 16 x 40
grid and cut 2D backbone, three classes) with the yaml's ROI_HEAD block.
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
import stack_pool_restatement as rs  # noqa: E402
from reference_loader import (MODEL_UTILS, ROI_HEAD, as_np as _np, cpu_torch, extension_stubs, load, model_yaml,  # noqa: E402
                              randomise, reference_root, second_settings, shapes, state, write_state_dict)
from pdanet_amd.config import to_attr  # noqa: E402

F32, I32 = np.float32, np.int32
BACKBONE_CHANNELS = {'x_conv1': 16, 'x_conv2': 32, 'x_conv3': 64, 'x_conv4': 64}


def _starts(cnt, rows_cnt):
    """start of its scene in the stacked features, for every row of the stacked centres"""
    start = np.cumsum(cnt) - cnt
    return np.repeat(start, rows_cnt)


class Stub(types.ModuleType):
    def __init__(self):
        super().__init__("pointnet2_stack_cuda")

    @staticmethod
    def voxel_query_wrapper(M, R1, R2, R3, nsample, radius, z_range, y_range, x_range, new_xyz, xyz, new_coords, point_indices, idx):
        rs.voxel_query(M, R1, R2, R3, nsample, radius, z_range, y_range, x_range, _np(new_xyz), _np(xyz), _np(new_coords),
                       _np(point_indices), _np(idx))
        return 1

    @staticmethod
    def group_points_wrapper(B, M, C, nsample, features, features_batch_cnt, idx, idx_batch_cnt, out):
        rows = _np(idx).astype(np.int64) + _starts(_np(features_batch_cnt), _np(idx_batch_cnt))[:, None]
        _np(out)[...] = _np(features)[rows].transpose(0, 2, 1)
        return 1

    @staticmethod
    def group_points_grad_wrapper(B, M, C, N, nsample, grad_out, idx, idx_batch_cnt, features_batch_cnt, grad_features):
        rows = _np(idx).astype(np.int64) + _starts(_np(features_batch_cnt), _np(idx_batch_cnt))[:, None]
        acc = np.zeros((N, C), np.float64)
        np.add.at(acc, rows.reshape(-1), _np(grad_out).transpose(0, 2, 1).reshape(-1, C).astype(np.float64))
        _np(grad_features)[...] = acc.astype(F32)
        return 1


def load_reference(root):
    """-> (voxel_pool_modules, voxelrcnn_head, common_utils) of the reference, as pcdet_ref.*"""
    cpu_torch()
    stack = "ops.pointnet2.pointnet2_stack."
    needed = load(root, "pcdet_ref", MODEL_UTILS + ROI_HEAD + [stack + "pointnet2_utils", stack + "voxel_query_utils"],
                  stubs=extension_stubs({stack + "pointnet2_stack_cuda": Stub()}))
    vpm, head = load(root, "pcdet_ref", [stack + "voxel_pool_modules", "models.roi_heads.voxelrcnn_head"])
    return vpm, head, needed[MODEL_UTILS.index("utils.common_utils")]


# ---- geometry shared by the two parts: voxel size 1/4 on [0, 8) x [-4, 4) x [-2, 2) --------------------------------------
PCR = [0.0, -4.0, -2.0, 8.0, 4.0, 2.0]
VOXEL = [0.25, 0.25, 0.25]
GRID_XYZ = [32, 32, 16]


def sparse_level(rng, stride, per_scene, channels, B=2):
    """indices (N, 4) int32 [b, z, y, x] of a level downsampled by `stride`, features (N, C)"""
    nx, ny, nz = (g // stride for g in GRID_XYZ)
    rows = []
    for b in range(B):
        cells = np.sort(rng.choice(nx * ny * nz, per_scene[b], replace=False))
        rows.append(np.stack([np.full(per_scene[b], b), cells // (ny * nx), (cells // nx) % ny, cells % nx], axis=1))
    ind = np.concatenate(rows).astype(I32)
    return ind, rng.standard_normal((len(ind), channels)).astype(F32), [nz, ny, nx]


def pool_part(vpm, cu, rng, out):
    B, stride, c_in = 2, 2, 16
    ind, feat, shape = sparse_level(rng, stride, [300, 220], c_in)
    t = torch.from_numpy
    sp = types.SimpleNamespace(indices=t(ind), features=t(feat), batch_size=B, spatial_shape=shape)
    xyz = cu.get_voxel_centers(sp.indices[:, 1:4], stride, VOXEL, PCR).contiguous()
    v2p = cu.generate_voxel2pinds(sp)
    xyz_cnt = t(np.array([300, 220], I32))
    m_per = 150
    new_xyz = np.concatenate([rng.integers(0, 64, (B * m_per, 1)), rng.integers(-32, 32, (B * m_per, 1)),
                              rng.integers(-16, 16, (B * m_per, 1))], axis=1).astype(F32) / 8
    new_xyz[:5] += 40                                   # far outside the grid: empty balls
    new_xyz[m_per:m_per + 3, 2] -= 9
    coords = np.floor((new_xyz - np.array(PCR[:3], F32)) / np.array(VOXEL, F32) / stride)
    new_coords = np.concatenate([np.repeat(np.arange(B), m_per)[:, None], coords], axis=1).astype(I32)   # [b, x, y, z]
    new_cnt = t(np.array([m_per, m_per], I32))
    torch.manual_seed(11)
    mod = vpm.NeighborVoxelSAModuleMSG(query_ranges=[[2, 2, 2], [1, 1, 1]], radii=[1.25, 0.75], nsamples=[16, 4],
                                       mlps=[[c_in, 32, 32], [c_in, 64, 32]], pool_method='max_pool')
    randomise(mod, rng)
    state(mod, "pool_", out)
    grad_out = rng.standard_normal((B * m_per, 64)).astype(F32)
    out.update(pool_indices=ind, pool_features=feat, pool_spatial_shape=np.array(shape, I32), pool_xyz=xyz.numpy(),
               pool_xyz_cnt=xyz_cnt.numpy(), pool_new_xyz=new_xyz, pool_new_cnt=new_cnt.numpy(), pool_new_coords=new_coords,
               pool_v2p=v2p.numpy(), pool_grad_out=grad_out, pool_stride=np.int32(stride))
    args = dict(xyz=xyz, xyz_batch_cnt=xyz_cnt, new_xyz=t(new_xyz), new_xyz_batch_cnt=new_cnt, new_coords=t(new_coords),
                voxel2point_indices=v2p)
    mod.eval()
    with torch.no_grad():
        out["pool_out_eval"] = mod(features=t(feat.copy()), **args).numpy()
    mod.train()
    f = t(feat.copy()).requires_grad_(True)
    res = mod(features=f, **args)
    (res * t(grad_out)).sum().backward()
    out["pool_out_train"] = res.detach().numpy()
    out["pool_grad_features"] = f.grad.numpy()
    for k, p in mod.named_parameters():
        out["pool_grad." + k] = p.grad.numpy().copy()
    for k, v in mod.named_buffers():
        out["pool_after." + k] = v.detach().numpy().copy()
    idx = np.zeros((B * m_per, 16), I32)
    zyx = np.ascontiguousarray(new_coords[:, [0, 3, 2, 1]])
    rs.voxel_query(B * m_per, *shape, 16, 1.25, 2, 2, 2, new_xyz, xyz.numpy(), zyx, v2p.numpy(), idx)
    print("pool: centres", B * m_per, "empty balls", int((idx[:, 0] < 0).sum()), "full balls", int((idx[:, 15] != idx[:, 0]).sum()))


HEAD_CFG = {
    'CLASS_AGNOSTIC': True, 'SHARED_FC': [32, 32], 'CLS_FC': [32, 32], 'REG_FC': [32, 32], 'DP_RATIO': 0.0,
    'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                             'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
                   'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 2048,
                            'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.7}},
    'ROI_GRID_POOL': {'FEATURES_SOURCE': ['x_conv2', 'x_conv3'], 'PRE_MLP': True, 'GRID_SIZE': 4, 'POOL_LAYERS': {
        'x_conv2': {'MLPS': [[32, 8]], 'QUERY_RANGES': [[2, 2, 2]], 'POOL_RADIUS': [1.25], 'NSAMPLE': [16], 'POOL_METHOD': 'max_pool'},
        'x_conv3': {'MLPS': [[64, 8]], 'QUERY_RANGES': [[1, 1, 1]], 'POOL_RADIUS': [1.5], 'NSAMPLE': [8], 'POOL_METHOD': 'max_pool'}}},
    'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5, 'SAMPLE_ROI_BY_EACH_CLASS': True,
                      'CLS_SCORE_TYPE': 'roi_iou', 'CLS_FG_THRESH': 0.75, 'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1,
                      'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55},
    'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                    'GRID_3D_IOU_LOSS': False,
                    'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,
                                     'rcnn_iou3d_weight': 1.0, 'code_weights': [1.0] * 7}},
}


def head_part(head_mod, rng, out):
    B, n_roi = 2, 6
    t = torch.from_numpy
    levels = {}
    for name, stride, per_scene in (('x_conv2', 2, [300, 220]), ('x_conv3', 4, [120, 90])):
        ind, feat, shape = sparse_level(rng, stride, per_scene, BACKBONE_CHANNELS[name])
        levels[name] = (ind, feat, shape, stride)
        out["head_%s_indices" % name], out["head_%s_features" % name] = ind, feat
        out["head_%s_spatial_shape" % name] = np.array(shape, I32)
    rois = np.zeros((B, n_roi, 7), F32)
    rois[..., 0] = rng.integers(8, 56, (B, n_roi)) / 8
    rois[..., 1] = rng.integers(-24, 24, (B, n_roi)) / 8
    rois[..., 2] = rng.integers(-8, 8, (B, n_roi)) / 8
    rois[..., 3:6] = rng.integers(1, 4, (B, n_roi, 3))
    rois[1, -1] = 0                                     # a zero-padded RoI row
    out["head_rois"] = rois
    out["head_cfg"] = np.array(json.dumps(HEAD_CFG))
    torch.manual_seed(12)
    head = head_mod.VoxelRCNNHead(backbone_channels=BACKBONE_CHANNELS, model_cfg=to_attr(copy.deepcopy(HEAD_CFG)),
                                  point_cloud_range=np.array(PCR), voxel_size=VOXEL, num_class=1)
    randomise(head, rng)
    with torch.no_grad():                               # the reference's std 0.001 would leave the predictions at zero
        head.cls_pred_layer.weight.normal_(0, 0.3, generator=torch.Generator().manual_seed(5))
        head.reg_pred_layer.weight.normal_(0, 0.1, generator=torch.Generator().manual_seed(6))
    state(head, "head_", out)

    def batch():
        feats = {k: types.SimpleNamespace(indices=t(v[0]), features=t(v[1].copy()), batch_size=B, spatial_shape=v[2])
                 for k, v in levels.items()}
        return {'batch_size': B, 'rois': t(rois.copy()), 'roi_scores': torch.zeros(B, n_roi),
                'roi_labels': torch.ones(B, n_roi, dtype=torch.long), 'multi_scale_3d_features': feats,
                'multi_scale_3d_strides': {k: v[3] for k, v in levels.items()}}

    head.eval()
    with torch.no_grad():
        bd = batch()
        out["head_pooled_eval"] = head.roi_grid_pool(bd).numpy()
        bd = head(batch())
        out["head_batch_cls_preds"], out["head_batch_box_preds"] = bd['batch_cls_preds'].numpy(), bd['batch_box_preds'].numpy()
    head.train()
    pooled = head.roi_grid_pool(batch())
    shared = head.shared_fc_layer(pooled.view(pooled.size(0), -1))
    out["head_pooled_train"] = pooled.detach().numpy()
    out["head_rcnn_cls_train"] = head.cls_pred_layer(head.cls_fc_layers(shared)).detach().numpy()
    out["head_rcnn_reg_train"] = head.reg_pred_layer(head.reg_fc_layers(shared)).detach().numpy()
    print("head: pooled", out["head_pooled_train"].shape, "nonzero share", float((out["head_pooled_train"] != 0).mean()))


def state_dict_part(root, head_mod):
    roi_cfg = model_yaml(root, "kitti_models/voxel_rcnn_car.yaml")["MODEL"]["ROI_HEAD"]
    second = second_settings()
    ds = second["config"]["dataset"]
    head = head_mod.VoxelRCNNHead(backbone_channels=BACKBONE_CHANNELS, model_cfg=to_attr(copy.deepcopy(roi_cfg)),
                                  point_cloud_range=np.array(ds["point_cloud_range"]), voxel_size=ds["voxel_size"], num_class=1)
    model_cfg = dict(second["config"]["MODEL"], NAME="VoxelRCNN", ROI_HEAD=roi_cfg)
    write_state_dict("voxel_rcnn_state_dict.json",
                     {"config": {"MODEL": model_cfg, "dataset": ds, "grid_size": second["config"]["grid_size"]},
                      "VoxelRCNNHead": shapes(head), "VoxelRCNN": second["SECONDNet"] + shapes(head, "roi_head.")})


def main():
    root = reference_root()
    vpm, head_mod, cu = load_reference(root)
    rng = np.random.default_rng(2025)
    out = {}
    pool_part(vpm, cu, rng, out)
    head_part(head_mod, rng, out)
    path = os.path.join(HERE, "voxel_rcnn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    state_dict_part(root, head_mod)


if __name__ == "__main__":
    main()
