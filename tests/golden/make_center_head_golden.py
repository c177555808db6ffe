#!/usr/bin/env python
"""Generates tests/golden/center_head.npz: the REFERENCE's CenterPoint pillar tail run on synthetic batches on CPU tensors --
PointPillarScatter, CenterHead.assign_targets, get_loss with its gradients, generate_predicted_boxes with the intermediate
results of _topk, decode_bbox_from_heatmap and class_agnostic_nms, and the state-dict keys of CenterHead and
BaseBEVBackbone.

The reference's own center_head.py, centernet_utils.py, loss_utils.py, model_nms_utils.py, pointpillar_scatter.py and
base_bev_backbone.py are loaded as pcdet_ref.* through reference_loader.py: numba (not installed) is a stub whose jit is an
identity decorator, iou3d_nms_cuda is bound to the repository's C oracle.  gt_boxes is
cloned before each call, because assign_targets writes the head-local class index back into its argument.

Two configurations on a map of W = 48, H = 40, B = 2 (not square, so that an x / y swap shows):
  a  the Waymo yaml's head: one head of three classes, stride 1, 8-column boxes;
  b  two heads [[A], [B, C]], stride 4, 'vel' in HEAD_ORDER, 10-column boxes, NUM_MAX_OBJS 8, MAX_OBJ_PER_SAMPLE 64,
     NMS_POST_MAXSIZE 16.
Three batches each: x = [rich scene, scene with class A only], y = [empty scene, class A only], z = [empty, empty] (the
focal loss's num_pos == 0 branch).  The rich scene is the list RICH.  The predictions are drawn once per
configuration and shared by its three batches.

The regression loss of the reference turns NaN as soon as one target is NaN (its `gt_regr * mask` is NaN * 0), so the NaN
velocity targets of configuration b are recorded twice: `loss_nan_*` is the reference on the targets as they are (NaN), and
the loss and gradients every test compares against are the reference on targets whose NaN entries are replaced by the
prediction at that entry's cell -- |pred - pred| = 0 with gradient sign(0) = 0, which is the rule `mask times not-NaN of
the target` that _reg_loss states.

The maker asserts on its own inputs: every float64 radius lies at least 1e-3 from an integer; the selected top-K scores and
the next one in rank are pairwise distinct; no decoded centre lies within 1e-4 of a face of POST_CENTER_LIMIT_RANGE; no
pair of boxes that enter the NMS has a BEV IoU within 1e-4 of NMS_THRESH.

Run with the reference checkout:  python tests/golden/make_center_head_golden.py /path/to/reference
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from reference_loader import MODEL_UTILS, cpu_torch, extension_stubs, load, reference_root, stub_numba  # noqa: E402
import oracle  # noqa: E402
from pdanet_amd.config import to_attr  # noqa: E402

OUT = os.path.join(HERE, "center_head.npz")
W, H, B = 48, 40, 2
# the reference's center_head, centernet_utils, model_nms_utils, base_bev_backbone and pointpillar_scatter, once loaded
CH = CU = NMS = BEV = PPS = None


def load_reference(root):
    global CH, CU, NMS, BEV, PPS
    cpu_torch()
    stub_numba()
    load(root, "pcdet_ref", MODEL_UTILS, stubs=extension_stubs())
    NMS, CU, CH, BEV, PPS = load(root, "pcdet_ref", [
        "models.model_utils.model_nms_utils", "models.model_utils.centernet_utils", "models.dense_heads.center_head",
        "models.backbones_2d.base_bev_backbone", "models.backbones_2d.map_to_bev.pointpillar_scatter"])


CLASS_NAMES = ['A', 'B', 'C']
HEAD_DICT = {'center': {'out_channels': 2, 'num_conv': 2}, 'center_z': {'out_channels': 1, 'num_conv': 2},
             'dim': {'out_channels': 3, 'num_conv': 2}, 'rot': {'out_channels': 2, 'num_conv': 2}}
CONFIGS = {
    # centerpoint_dyn_pillar_1x.yaml DENSE_HEAD on a 48 x 40 map: voxels of 0.32 m, stride 1
    'a': {
        'point_cloud_range': [-7.68, -6.4, -2.0, 7.68, 6.4, 4.0], 'voxel_size': [0.32, 0.32, 6.0], 'gt_cols': 8,
        'head': {
            'CLASS_AGNOSTIC': False, 'CLASS_NAMES_EACH_HEAD': [['A', 'B', 'C']], 'SHARED_CONV_CHANNEL': 64,
            'USE_BIAS_BEFORE_NORM': True, 'NUM_HM_CONV': 2,
            'SEPARATE_HEAD_CFG': {'HEAD_ORDER': ['center', 'center_z', 'dim', 'rot'], 'HEAD_DICT': HEAD_DICT},
            'TARGET_ASSIGNER_CONFIG': {'FEATURE_MAP_STRIDE': 1, 'NUM_MAX_OBJS': 500, 'GAUSSIAN_OVERLAP': 0.1, 'MIN_RADIUS': 2},
            'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0, 'code_weights': [1.0] * 8}},
            'POST_PROCESSING': {'SCORE_THRESH': 0.1, 'POST_CENTER_LIMIT_RANGE': [-7.0, -6.0, -1.05, 7.0, 6.0, 1.05],
                                'MAX_OBJ_PER_SAMPLE': 500,
                                'NMS_CONFIG': {'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.7, 'NMS_PRE_MAXSIZE': 4096,
                                               'NMS_POST_MAXSIZE': 500}}}},
    # two heads, voxels of 0.1 m, stride 4, velocities
    'b': {
        'point_cloud_range': [-9.6, -8.0, -5.0, 9.6, 8.0, 3.0], 'voxel_size': [0.1, 0.1, 8.0], 'gt_cols': 10,
        'head': {
            'CLASS_AGNOSTIC': False, 'CLASS_NAMES_EACH_HEAD': [['A'], ['B', 'C']], 'SHARED_CONV_CHANNEL': 32,
            'USE_BIAS_BEFORE_NORM': False, 'NUM_HM_CONV': 2,
            'SEPARATE_HEAD_CFG': {'HEAD_ORDER': ['center', 'center_z', 'dim', 'rot', 'vel'],
                                  'HEAD_DICT': dict(HEAD_DICT, vel={'out_channels': 2, 'num_conv': 2})},
            'TARGET_ASSIGNER_CONFIG': {'FEATURE_MAP_STRIDE': 4, 'NUM_MAX_OBJS': 8, 'GAUSSIAN_OVERLAP': 0.1, 'MIN_RADIUS': 2},
            'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 0.25,
                                             'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]}},
            'POST_PROCESSING': {'SCORE_THRESH': 0.3, 'POST_CENTER_LIMIT_RANGE': [-9.0, -7.5, -1.05, 9.0, 7.5, 1.05],
                                'MAX_OBJ_PER_SAMPLE': 64,
                                'NMS_CONFIG': {'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.2, 'NMS_PRE_MAXSIZE': 1000,
                                               'NMS_POST_MAXSIZE': 16}}}},
}


def make_head(cfg, input_channels=16):
    grid = np.round((np.array(cfg['point_cloud_range'][3:]) - np.array(cfg['point_cloud_range'][:3])) / np.array(cfg['voxel_size'])).astype(np.int64)
    return CH.CenterHead(model_cfg=to_attr(cfg['head']), input_channels=input_channels, num_class=3, class_names=CLASS_NAMES,
                         grid_size=grid, point_cloud_range=np.array(cfg['point_cloud_range']), voxel_size=cfg['voxel_size'],
                         predict_boxes_when_training=False)


# ---- scenes, in map cells -------------------------------------------------------------------------------------------------------
# (centre x, centre y, dx, dy in cells, class 1..3); the order is the row order, and under configuration b only the first
# 8 rows of a head are kept, so the rows a test depends on come first
RICH = [
    (25.1, 25.2, 3.0, 2.0, 2), (25.5, 25.5, 2.5, 2.5, 2), (25.8, 25.1, 2.0, 3.0, 2),      # three objects of B in cell (25, 25)
    (10.2, 10.3, 4.0, 2.0, 1), (10.7, 10.6, 3.5, 2.2, 1),                                  # two of A in cell (10, 10)
    (0.6, 20.3, 6.0, 3.0, 1),                                                              # clipped by the left border
    (47.2, 10.7, 5.0, 4.0, 2),                                                             # right border
    (20.4, 0.3, 4.0, 6.0, 3),                                                              # top border
    None,                                                                                  # a zero row in the middle
    (30.6, 39.4, 5.5, 3.0, 1),                                                             # bottom border
    (47.6, 39.7, 6.0, 6.0, 2),                                                             # the corner
    (-3.2, 15.5, 3.0, 3.0, 3),                                                             # outside on the left: clamped to 0
    (51.0, 45.0, 3.0, 2.0, 1),                                                             # outside on the right: W - 0.5, H - 0.5
    (33.3, 12.4, 0.0, 2.0, 2),                                                             # dx = 0: the slot stays zero
    (14.3, 30.2, 3.0, 2.0, 1), (16.4, 30.9, 3.2, 2.1, 1),                                  # overlapping Gaussians of A
    (38.5, 22.5, 4.0, 3.0, 1), (40.1, 23.4, 4.0, 3.0, 3),                                  # overlapping Gaussians of A and C
    (24.4, 18.6, 60.0, 50.0, 3),                                                           # r = 23 > 16
    (5.5, 34.5, 2.0, 2.0, 3), (8.5, 5.5, 2.0, 1.0, 2), (42.5, 3.5, 1.0, 2.0, 3), (12.5, 21.5, 2.2, 2.2, 2),
    (36.5, 31.5, 3.0, 1.5, 3), (28.5, 8.5, 1.5, 3.0, 2),                                    # head [B, C] well past 8 objects
]
ONLY_A = [(12.3, 9.4, 4.0, 2.0, 1), (30.8, 28.1, 3.0, 3.0, 1), None, (44.4, 35.6, 5.0, 2.5, 1)]
M_ROWS = 28


def scene(rng, rows, cfg):
    """gt rows (M_ROWS, gt_cols) of a scene given in map cells, zero-padded at the end and at the None entries."""
    cols = cfg['gt_cols']
    stride = cfg['head']['TARGET_ASSIGNER_CONFIG']['FEATURE_MAP_STRIDE']
    cell = np.array(cfg['voxel_size'][:2]) * stride
    g = np.zeros((M_ROWS, cols), np.float64)
    for i, r in enumerate(rows):
        if r is None:
            continue
        g[i, 0] = cfg['point_cloud_range'][0] + r[0] * cell[0]
        g[i, 1] = cfg['point_cloud_range'][1] + r[1] * cell[1]
        g[i, 2] = rng.uniform(-1.0, 1.0)
        g[i, 3], g[i, 4], g[i, 5] = r[2] * cell[0], r[3] * cell[1], rng.uniform(1.0, 2.0)
        g[i, 6] = rng.uniform(-np.pi, np.pi)
        if cols == 10:
            g[i, 7:9] = rng.standard_normal(2)
            if i in (1, 3, 6):                               # NaN velocities, the first of them at the three-object cell
                g[i, 7:9] = np.nan
            if i == 4:
                g[i, 8] = np.nan
        g[i, -1] = r[4]
    return g.astype(np.float32)


def radius64(dx, dy, o):
    """gaussian_radius in float64."""
    b1, c1 = dx + dy, dx * dy * (1 - o) / (1 + o)
    r1 = (b1 + np.sqrt(b1 ** 2 - 4 * c1)) / 2
    b2, c2 = 2 * (dx + dy), (1 - o) * dx * dy
    r2 = (b2 + np.sqrt(b2 ** 2 - 16 * c2)) / 2
    a3, b3, c3 = 4 * o, -2 * o * (dx + dy), (o - 1) * dx * dy
    r3 = (b3 + np.sqrt(b3 ** 2 - 4 * a3 * c3)) / 2
    return min(r1, r2, r3)


def check_radii(gt, cfg):
    t = cfg['head']['TARGET_ASSIGNER_CONFIG']
    big = 0
    for row in gt.reshape(-1, gt.shape[-1]).astype(np.float64):
        if row[-1] == 0 or row[3] <= 0 or row[4] <= 0:
            continue
        r = radius64(row[3] / cfg['voxel_size'][0] / t['FEATURE_MAP_STRIDE'], row[4] / cfg['voxel_size'][1] / t['FEATURE_MAP_STRIDE'],
                     t['GAUSSIAN_OVERLAP'])
        assert abs(r - round(r)) >= 1e-3, (row, r)
        big = max(big, int(r))
    return big


def predictions(rng, cfg, heatmaps):
    """One pred_dict per head: heat-map logits N(-4.5, 1.5) with a few beyond +-10 (at a positive cell and elsewhere), the
    regression maps N(0, 0.5) rounded to float16 values."""
    preds = []
    for h, names in enumerate(cfg['head']['CLASS_NAMES_EACH_HEAD']):
        c = len(names)
        d = {'hm': (rng.standard_normal((B, c, H, W)) * 1.5 - 4.5).astype(np.float32)}
        for name, spec in cfg['head']['SEPARATE_HEAD_CFG']['HEAD_DICT'].items():
            d[name] = (rng.standard_normal((B, spec['out_channels'], H, W)) * 0.5).astype(np.float16).astype(np.float32)
        pos = np.argwhere(heatmaps[h] == 1)
        extremes = [12.0, -12.5, 11.0, -13.0, 13.5, -11.5, 10.5, -10.25]
        for j, v in enumerate(extremes):
            if j < 4 and len(pos) > j:
                d['hm'][tuple(pos[j])] = v                   # the clamp at cells with gt == 1, both sides
            else:
                d['hm'][j % B, j % c, 3 + 4 * j, 5 + 5 * j] = v
        preds.append(d)
    return preds


def bev_iou(boxes):
    n = boxes.shape[0]
    ov = np.zeros((n, n), np.float32)
    b7 = np.ascontiguousarray(boxes[:, :7])
    oracle.boxes_overlap_bev_gpu(b7, b7, ov)
    area = (boxes[:, 3] * boxes[:, 4]).astype(np.float64)
    return ov / np.maximum(area[:, None] + area[None, :] - ov, 1e-8)


def run_batch(out, p, cfg, head, gt, rng, preds_np=None):
    """Everything the reference computes for one batch, stored under prefix p.  preds_np: the predictions of an earlier
    batch of the configuration (they are stored once); None: drawn here and stored under the configuration's name."""
    t_cfg = cfg['head']['TARGET_ASSIGNER_CONFIG']
    out[p + 'gt_boxes'] = gt
    out[p + 'max_radius'] = np.int64(check_radii(gt, cfg))
    targets = head.assign_targets(torch.from_numpy(gt.copy()), feature_map_size=(H, W))
    n_heads = len(targets['heatmaps'])
    for h in range(n_heads):
        for key in ('heatmaps', 'target_boxes', 'inds', 'masks'):
            out['%st%d_%s' % (p, h, key)] = targets[key][h].numpy().copy()
    if preds_np is None:
        preds_np = predictions(rng, cfg, [targets['heatmaps'][h].numpy() for h in range(n_heads)])
        for h in range(n_heads):
            for k, v in preds_np[h].items():             # the regression maps hold float16 values and are stored so
                out['%s_p%d_%s' % (p[0], h, k)] = v if k == 'hm' else v.astype(np.float16)
    order = cfg['head']['SEPARATE_HEAD_CFG']['HEAD_ORDER']

    def loss_run(target_boxes):
        preds = [{k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in d.items()} for d in preds_np]
        head.forward_ret_dict = {'pred_dicts': [dict(d) for d in preds],
                                 'target_dicts': dict(targets, target_boxes=target_boxes)}
        loss, tb = head.get_loss()
        if torch.isfinite(loss):
            loss.backward()
        return preds, loss, tb

    # the reference as it is (NaN with NaN targets), then with each NaN target replaced by the prediction at its cell
    _, loss_nan, tb_nan = loss_run(targets['target_boxes'])
    out[p + 'loss_nan'] = np.float32(loss_nan.item())
    filled = []
    for h in range(n_heads):
        tb_h = targets['target_boxes'][h].clone()
        cat = torch.cat([torch.from_numpy(preds_np[h][k]) for k in order], dim=1)
        pred = CU._transpose_and_gather_feat(cat, targets['inds'][h])
        nan = torch.isnan(tb_h)
        tb_h[nan] = pred[nan]
        filled.append(tb_h)
    out[p + 'n_nan_targets'] = np.int64(sum(int(torch.isnan(t).sum()) for t in targets['target_boxes']))
    preds, loss, tb = loss_run(filled)
    assert torch.isfinite(loss)
    out[p + 'loss'] = np.float32(loss.item())
    for h in range(n_heads):
        out['%sl%d_hm_loss' % (p, h)] = np.float64(tb['hm_loss_head_%d' % h])
        out['%sl%d_loc_loss' % (p, h)] = np.float64(tb['loc_loss_head_%d' % h])
        for k, v in preds_np[h].items():
            out['%sg%d_%s' % (p, h, k)] = preds[h][k].grad.numpy().copy()

    # decoding: _topk, decode_bbox_from_heatmap, the NMS of every (head, scene), then the reference's own composition
    pp = cfg['head']['POST_PROCESSING']
    K = pp['MAX_OBJ_PER_SAMPLE']
    limit = torch.tensor(pp['POST_CENTER_LIMIT_RANGE']).float()
    with torch.no_grad():
        for h in range(n_heads):
            d = {k: torch.from_numpy(v.copy()) for k, v in preds_np[h].items()}
            hm = d['hm'].sigmoid()
            flat = np.sort(hm.numpy().reshape(B, -1), axis=1)[:, ::-1][:, :K + 1]
            assert (np.diff(flat, axis=1) < 0).all(), "ties among the selected scores"
            scores, inds, cls, ys, xs = CU._topk(hm, K=K)
            out['%sd%d_topk_inds' % (p, h)] = inds.numpy().copy()
            out['%sd%d_topk_cls' % (p, h)] = cls.numpy().copy()
            out['%sd%d_topk_scores' % (p, h)] = scores.numpy().copy()
            dec = CU.decode_bbox_from_heatmap(
                heatmap=hm, rot_cos=d['rot'][:, 0:1], rot_sin=d['rot'][:, 1:2], center=d['center'], center_z=d['center_z'],
                dim=d['dim'].exp(), vel=d.get('vel') if 'vel' in order else None, point_cloud_range=head.point_cloud_range,
                voxel_size=head.voxel_size, feature_map_stride=head.feature_map_stride, K=K, circle_nms=False,
                score_thresh=pp['SCORE_THRESH'], post_center_limit_range=limit)
            for s, sd in enumerate(dec):
                boxes = sd['pred_boxes'].numpy()
                out['%sd%d_s%d_boxes' % (p, h, s)] = boxes.copy()
                out['%sd%d_s%d_scores' % (p, h, s)] = sd['pred_scores'].numpy().copy()
                out['%sd%d_s%d_labels' % (p, h, s)] = sd['pred_labels'].numpy().copy()
                selected, _ = NMS.class_agnostic_nms(box_scores=sd['pred_scores'], box_preds=sd['pred_boxes'],
                                                     nms_config=to_attr(pp['NMS_CONFIG']), score_thresh=None)
                out['%sd%d_s%d_keep' % (p, h, s)] = np.asarray(selected.numpy() if torch.is_tensor(selected) else selected, np.int64).copy()
                if len(boxes) > 1:
                    iou = bev_iou(boxes)
                    assert (np.abs(iou - pp['NMS_CONFIG']['NMS_THRESH']) >= 1e-4).all(), "a BEV IoU next to NMS_THRESH"
            # every decoded centre, masked or not, against the faces of the limit range
            allc = CU.decode_bbox_from_heatmap(
                heatmap=hm, rot_cos=d['rot'][:, 0:1], rot_sin=d['rot'][:, 1:2], center=d['center'], center_z=d['center_z'],
                dim=d['dim'].exp(), vel=None, point_cloud_range=head.point_cloud_range, voxel_size=head.voxel_size,
                feature_map_stride=head.feature_map_stride, K=K, circle_nms=False, score_thresh=None,
                post_center_limit_range=torch.tensor([-1e9] * 3 + [1e9] * 3))
            for sd in allc:
                c = sd['pred_boxes'][:, :3].numpy().astype(np.float64)
                lim = np.array(pp['POST_CENTER_LIMIT_RANGE'], np.float64)
                assert (np.abs(c - lim[:3]) >= 1e-4).all() and (np.abs(c - lim[3:]) >= 1e-4).all(), "a centre on a face"
        final = head.generate_predicted_boxes(B, [{k: torch.from_numpy(v.copy()) for k, v in d.items()} for d in preds_np])
        for s, fd in enumerate(final):
            for k, v in fd.items():
                out['%sf_s%d_%s' % (p, s, k)] = v.numpy().copy()
    return targets, preds_np


def scatter_case(out, rng):
    """PointPillarScatter on 150 pillars (three tiles of 64, the last one partial) of 70 channels (two chunks of 64, the last
    one partial) on a 13 x 10 grid, two scenes, with its backward through autograd."""
    n, C, W, H = 150, 70, 13, 10
    cells = np.sort(rng.permutation(B * H * W)[:n])          # distinct cells, ascending as DynamicPillarVFE emits them
    coords = np.zeros((n, 4), np.int32)
    coords[:, 0], coords[:, 2], coords[:, 3] = cells // (H * W), (cells % (H * W)) // W, cells % W
    feats = torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32)).requires_grad_(True)
    mod = PPS.PointPillarScatter(to_attr({'NUM_BEV_FEATURES': C}), grid_size=(W, H, 1))
    bd = mod({'pillar_features': feats, 'voxel_coords': torch.from_numpy(coords)})
    grad = torch.from_numpy(rng.standard_normal((B, C, H, W)).astype(np.float32))
    bd['spatial_features'].backward(grad)
    out['sc_features'], out['sc_coords'], out['sc_grid'] = feats.detach().numpy(), coords, np.array([W, H, 1], np.int64)
    out['sc_out'], out['sc_grad_out'], out['sc_grad_features'] = bd['spatial_features'].detach().numpy(), grad.numpy(), feats.grad.numpy()


def main():
    load_reference(reference_root())
    rng = np.random.default_rng(20261018)
    torch.manual_seed(11)
    out = {'configs': np.array(json.dumps(CONFIGS)), 'class_names': np.array(CLASS_NAMES), 'map_hw': np.array([H, W], np.int64)}
    for name, cfg in CONFIGS.items():
        head = make_head(cfg)
        out['keys_%s' % name] = np.array(list(head.state_dict().keys()), dtype='<U80')
        rich, only_a = scene(rng, RICH, cfg), scene(rng, ONLY_A, cfg)
        empty = np.zeros_like(rich)
        preds_np = None
        for tag, gt in (('x', np.stack([rich, only_a])), ('y', np.stack([empty, only_a])), ('z', np.stack([empty, empty]))):
            targets, preds_np = run_batch(out, '%s%s_' % (name, tag), cfg, head, gt, rng, preds_np)
            print(name, tag, [int(m.sum()) for m in targets['masks']], 'max radius', int(out['%s%s_max_radius' % (name, tag)]),
                  'loss', float(out['%s%s_loss' % (name, tag)]), 'loss as the reference has it', float(out['%s%s_loss_nan' % (name, tag)]),
                  'kept', [[len(out['%s%s_d%d_s%d_keep' % (name, tag, h, s)]) for s in range(B)] for h in range(len(targets['masks']))])
    assert out['ax_max_radius'] > 16
    assert out['bx_n_nan_targets'] > 0 and np.isnan(out['bx_loss_nan'])
    bev_cfg = {'LAYER_NUMS': [3, 5, 5], 'LAYER_STRIDES': [1, 2, 2], 'NUM_FILTERS': [64, 128, 256], 'UPSAMPLE_STRIDES': [1, 2, 4],
               'NUM_UPSAMPLE_FILTERS': [128, 128, 128]}
    out['bev_cfg'] = np.array(json.dumps(bev_cfg))
    out['keys_bev'] = np.array(list(BEV.BaseBEVBackbone(to_attr(bev_cfg), 64).state_dict().keys()), dtype='<U80')
    scatter_case(out, rng)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 1 << 20


if __name__ == "__main__":
    main()
