#!/usr/bin/env python
"""Generates tests/golden/anchor_head_coded.npz and anchor_head_coded_state_dicts.json: the REFERENCE's own AnchorHeadMulti,
AxisAlignedTargetAssigner, ResidualCoder (encode_angle_by_sincos, code_size 9), WeightedL1Loss and post_processing over
multi_classes_nms, imported from where they lie and run on CPU tensors, through the stubs of reference_loader.py and the
helpers of make_anchor_head_multi_golden.py (same geometry: range [0, -3.6, -3, 8.8, 3.6, 1], voxels of 0.4 m, stride 2, an
11 x 9 map, B = 2, M = 12; no row count a multiple of 64).  Nothing of the reference is copied; what is committed is data.

    python tests/golden/make_anchor_head_coded_golden.py <checkout of the reference>

Three configurations:
  n  the nuScenes head in small: five classes in the heads [c0], [c1, c2], [c3, c4], SEPARATE_MULTIHEAD, SHARED_CONV_NUM_FILTER,
     SEPARATE_REG_CONFIG with REG_LIST reg:2 height:1 size:3 angle:2 velo:2, code_size 9 with encode_angle_by_sincos (10 code
     columns), WeightedL1Loss, code_weights 8 x 1.0 + 2 x 0.2, pos_cls_weight 1, neg_cls_weight 2, no direction classifier;
     gt (B, M, 10); 5 x 198 = 990 anchors;
  s  sincos alone: code_size 7 (8 code columns), the heads of configuration c there with SEPARATE_MULTIHEAD False, smooth L1,
     non-uniform code_weights; gt (B, M, 8); 891 anchors;
  v  velocities alone: code_size 9 without sincos (9 code columns), the heads of configuration b there with the direction
     classifier (sine difference and direction bins on 9-wide rows), smooth L1; gt (B, M, 10); 891 anchors.
Batches x, y, z and the rich scene are make_anchor_head_multi_golden.py's (twin boxes, a square box tying two rotations, a forced
positive, a box overlapping nothing, a heading past pi / 4, an interior zero row, trailing zero rows), asserted as there.  With
velocities: gt rows carry velocities that are float16 values; row 5 of the rich scene has both NaN, row 7 has vx NaN only, row 2
of the one-class scene has vy NaN; the twins carry the same velocity; zero rows stay zero.  The maker asserts that at least two
positives have a NaN velocity target, one of them in one column only, and (n) that a positive's prediction equals its target
exactly in column 8: the kink of the L1 term.  The sincos codes of the predictions are drawn so that every row's
hypot(sin_t + sin(ra), cos_t + cos(ra)) >= 0.25; the minimum is recorded as <name>_min_hypot.

post_n: post_processing with MULTI_CLASSES_NMS over configuration n's heads with 9-column boxes, as post_a / post_b there:
scores a permutation of an even grid per column, pairwise 1e-5 apart and 1e-4 from the threshold, NMS_PRE_MAXSIZE 96 below some
column's rows above the threshold, NMS_POST_MAXSIZE 8 below some column's survivors, one column empty -- all asserted.

The json: the state-dict keys and shapes of configuration n's head, and of the two detectors of
nuscenes_models/cbgs_pp_multihead.yaml and cbgs_second_multihead.yaml (vfe, backbone_3d, backbone_2d, dense_head as
Detector3DTemplate names them) on small grids with the 2D backbone cut short, plus the settings they were built with.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from reference_loader import load, model_yaml, reference_root, shapes, stub_numba, write_state_dict  # noqa: E402
import make_anchor_head_multi_golden as base  # noqa: E402
import oracle  # noqa: E402
from pdanet_amd.config import to_attr  # noqa: E402

OUT = os.path.join(HERE, "anchor_head_coded.npz")
B, M, PCR, VOXEL, POST = base.B, base.M, base.PCR, base.VOXEL, base.POST
CLASS_NAMES = {'n': ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Truck'], 's': base.CLASS_NAMES, 'v': base.CLASS_NAMES}
MIN_HYPOT = 0.25


def target(**coder):
    return dict(base.TARGET, BOX_CODER_CONFIG=coder)


def n_generator():
    more = {'anchor_bottom_heights': [-1.6], 'align_center': False, 'feature_map_stride': 2, 'anchor_rotations': [0, 1.57]}
    return base.generator([[0.8, 0.6, 1.73]], [0, 1.57]) + [
        dict(more, class_name='Van', anchor_sizes=[[4.6, 1.9, 1.9]], matched_threshold=0.55, unmatched_threshold=0.4),
        dict(more, class_name='Truck', anchor_sizes=[[6.9, 2.5, 2.8]], matched_threshold=0.5, unmatched_threshold=0.35)]


def with_loss(cfg, reg_loss, **weights):
    cfg = json.loads(json.dumps(cfg))
    if reg_loss is not None:
        cfg['LOSS_CONFIG']['REG_LOSS_TYPE'] = reg_loss
    cfg['LOSS_CONFIG']['LOSS_WEIGHTS'].update(weights)
    return cfg


CONFIGS = {
    'n': with_loss(base.head_cfg(True, [{'HEAD_CLS_NAME': ['Car']}, {'HEAD_CLS_NAME': ['Pedestrian', 'Cyclist']},
                                        {'HEAD_CLS_NAME': ['Van', 'Truck']}], n_generator(), False, [1.0] * 8 + [0.2] * 2,
                                 SHARED_CONV_NUM_FILTER=8, TARGET_ASSIGNER_CONFIG=target(code_size=9, encode_angle_by_sincos=True),
                                 DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
                                 SEPARATE_REG_CONFIG={'NUM_MIDDLE_CONV': 1, 'NUM_MIDDLE_FILTER': 8,
                                                      'REG_LIST': ['reg:2', 'height:1', 'size:3', 'angle:2', 'velo:2']}),
                   'WeightedL1Loss', pos_cls_weight=1.0, neg_cls_weight=2.0),
    's': with_loss(base.head_cfg(False, base.CONFIGS['c']['RPN_HEAD_CFGS'], base.generator([[0.8, 0.6, 1.73], [0.6, 0.9, 1.5]],
                                                                                          [0, 1.57, 0.5]),
                                 False, [1.0, 1.0, 0.5, 1.0, 1.0, 2.0, 0.75, 1.25],
                                 TARGET_ASSIGNER_CONFIG=target(code_size=7, encode_angle_by_sincos=True)), 'WeightedSmoothL1Loss'),
    'v': with_loss(base.head_cfg(True, base.TWO_HEADS, base.generator([[0.8, 0.6, 1.73], [0.6, 0.9, 1.5]], [0, 1.57, 0.5]), True,
                                 [1.0, 1.0, 0.5, 1.0, 1.0, 2.0, 0.75, 0.2, 0.4], TARGET_ASSIGNER_CONFIG=target(code_size=9)), None),
}
LAYOUT = {'n': (10, 1, 2), 's': (8, 1, 0), 'v': (9, 0, 2)}      # code columns, sincos, extra


def make_head(mod, name):
    pcr, vs = np.array(PCR, np.float64), np.array(VOXEL, np.float64)
    grid = np.round((pcr[3:] - pcr[:3]) / vs).astype(np.int64)
    names = CLASS_NAMES[name]
    return mod.AnchorHeadMulti(model_cfg=to_attr(CONFIGS[name]), input_channels=16, num_class=len(names), class_names=names,
                               grid_size=grid, point_cloud_range=pcr, predict_boxes_when_training=False)


def seven(head):
    """The head's anchors without the zero columns the reference pads them with, for the helpers of the 7-column maker."""
    for a in head.anchors:
        assert not a[..., 7:].any(), "the padding of the anchors is not zero"
    return types.SimpleNamespace(anchors=[a[..., :7].contiguous() for a in head.anchors])


def with_velocities(gt8, extra, scene):
    """(M, 8) -> (M, 8 + extra): velocities that are float16 values behind the heading, NaN where the docstring says."""
    if extra == 0:
        return gt8
    rng = np.random.default_rng(100 + scene)
    vel = (np.round(rng.uniform(-4, 4, (M, extra)) * 8) / 8).astype(np.float32)
    vel[~gt8.any(axis=1)] = 0
    if scene == 0:
        vel[1] = vel[0]
        vel[5] = np.nan
        vel[7, 0] = np.nan
    else:
        vel[2, 1] = np.nan
    return np.concatenate([gt8[:, :7], vel, gt8[:, 7:]], axis=1).astype(np.float32)


def as_eight(gt):
    return np.ascontiguousarray(np.concatenate([gt[..., :7], gt[..., -1:]], axis=-1))


def predictions(rng, name, cfg, table, positives, first_targets):
    """As make_anchor_head_multi_golden.py: few distinct values, every one a float16; the sincos codes kept away from the
    origin of the atan2; n: one positive's column 8 equal to its target."""
    code, sincos, extra = LAYOUT[name]
    N, C = table.shape[0], len(CLASS_NAMES[name])
    cls = np.clip(np.round((rng.standard_normal((B, N, C)) - 6.0) * 4) / 4, -9, -2.5).astype(np.float32)
    cls[positives[0][:4], positives[1][:4], :] = np.array([2.5, -6.0, 0.25, -1.5], np.float32)[:, None]
    box = np.round(rng.standard_normal((B, N, code)) * 0.3 * 64) / 64
    keep = rng.random((B, N)) < 0.2
    keep[positives] = True
    box = (box * keep[..., None]).astype(np.float32)
    if sincos:
        ra = table[None, :, 6].astype(np.float64)
        near = np.hypot(box[..., 7] + np.sin(ra), box[..., 6] + np.cos(ra)) < MIN_HYPOT + 0.05
        box[near, 6:8] = 0
    kink = None
    if name == 'n':
        t = first_targets[positives][:, 8]
        i = int(np.nonzero(~np.isnan(t) & (t != 0))[0][0])
        kink = (int(positives[0][i]), int(positives[1][i]), 8)
        box[kink] = t[i]
        assert np.float32(np.float16(t[i])) == t[i]
    d = None
    if cfg.get('USE_DIRECTION_CLASSIFIER'):
        d = np.round(rng.standard_normal((B, N, 2)) * 8) / 8
        d[..., 1] = d[..., 0] + rng.choice([-1.5, -0.5, -0.125, 0.125, 0.75, 2.0], size=(B, N))
        d = d.astype(np.float32)
    return (cls, box, d), kink


def min_hypot(codes, table):
    ra = table[None, :, 6].astype(np.float64)
    return float(np.hypot(codes[..., 7].astype(np.float64) + np.sin(ra), codes[..., 6].astype(np.float64) + np.cos(ra)).min())


def post_case(out, name, head, template, table, rows, cols, gt, rng):
    """post_processing with MULTI_CLASSES_NMS on the per-head logits and the decoded 9-column boxes of random codes."""
    code, sincos, extra = LAYOUT[name]
    N, C = table.shape[0], len(CLASS_NAMES[name])
    thr = POST['SCORE_THRESH']
    logit_thr = np.log(thr / (1 - thr))
    cls = [np.stack([np.stack([rng.permutation(np.linspace(-4.0, 2.0, n)) + rng.uniform(0, 0.01) for _ in range(c)], axis=1)
                     for _ in range(B)]).astype(np.float32) for n, c in zip(rows, cols)]
    for x in cls:
        x[np.abs(x - logit_thr) < 0.01] += 0.02
    cls[-1][1, :, -1] -= 5.0                                                           # a column with nothing above the threshold
    codes = (rng.standard_normal((B, N, code)) * 0.2).astype(np.float32)
    assert min_hypot(codes, table) >= MIN_HYPOT
    with torch.no_grad():
        _, boxes = head.generate_predicted_boxes(B, [torch.from_numpy(v) for v in cls],
                                                 [torch.from_numpy(v) for v in base.split(codes, rows)], None)
    boxes = boxes.numpy().copy()
    assert boxes.shape == (B, N, 7 + extra)
    for x in cls:
        s = 1 / (1 + np.exp(-x.astype(np.float64)))
        assert np.abs(s - thr).min() >= 1e-4, "a score next to the threshold"
        for b in range(B):
            for k in range(x.shape[2]):
                live = np.sort(s[b, :, k][s[b, :, k] >= thr])
                assert len(live) < 2 or np.diff(live).min() >= 1e-5, "two scores of a column closer than 1e-5"
    batch = {'batch_size': B, 'batch_cls_preds': [torch.from_numpy(v.copy()) for v in cls],
             'batch_box_preds': torch.from_numpy(boxes.copy()), 'cls_preds_normalized': False,
             'multihead_label_mapping': [h.head_label_indices for h in head.rpn_heads], 'gt_boxes': torch.from_numpy(gt.copy())}
    fake = types.SimpleNamespace(model_cfg=to_attr({'POST_PROCESSING': POST}), num_class=C,
                                 generate_recall_record=template.Detector3DTemplate.generate_recall_record)
    with torch.no_grad():
        pred_dicts, recall = template.Detector3DTemplate.post_processing(fake, batch)
    pre, post = POST['NMS_CONFIG']['NMS_PRE_MAXSIZE'], POST['NMS_CONFIG']['NMS_POST_MAXSIZE']
    K = sum(cols) * post
    pb, ps, pl = np.zeros((B, K, 7 + extra), np.float32), np.zeros((B, K), np.float32), np.zeros((B, K), np.int64)
    counts = np.zeros(B, np.int32)
    for b, d in enumerate(pred_dicts):
        n = counts[b] = len(d['pred_scores'])
        pb[b, :n], ps[b, :n], pl[b, :n] = d['pred_boxes'].numpy(), d['pred_scores'].numpy(), d['pred_labels'].numpy()
    p = 'post_%s_' % name
    for h, x in enumerate(cls):
        out['%scls_%d' % (p, h)] = x
    out[p + 'boxes'], out[p + 'gt_boxes'] = boxes, gt
    out[p + 'pred_boxes'], out[p + 'pred_scores'], out[p + 'pred_labels'], out[p + 'num_pred'] = pb, ps, pl, counts
    out[p + 'recall'] = np.array(json.dumps({k: int(v) for k, v in recall.items()}))
    above = max(int((1 / (1 + np.exp(-x.astype(np.float64))) >= thr).sum(axis=1).max()) for x in cls)
    per_label = [np.bincount(pl[b, :counts[b]], minlength=C + 1) for b in range(B)]
    assert min(rows) > pre and above > pre, "no column is truncated by NMS_PRE_MAXSIZE"
    assert max(v.max() for v in per_label) == post, "no column reaches NMS_POST_MAXSIZE"
    assert per_label[1][C] == 0 and per_label[0][C] > 0, "the empty column"
    assert np.abs(pb[..., 7:]).max() > 0, "the velocity columns of the predictions"
    print(name, 'post: counts', counts, 'per label', per_label, 'recall', recall)


def state_dicts(root, multi, n_head):
    """The key lists: configuration n's head, and the two detectors on small grids with the 2D backbone cut short."""
    from make_second_state_dict import _spconv_stand_in
    _spconv_stand_in()
    stub_numba()
    if not hasattr(np, 'int'):
        np.int = int      # base_bev_backbone.py:60 names the alias numpy has dropped (an UPSAMPLE_STRIDES below 1)
    load(root, "pcdet_ref", ["utils.spconv_utils", "models.backbones_3d.vfe.vfe_template"])
    pvfe, b3d = load(root, "pcdet_ref", ["models.backbones_3d.vfe.pillar_vfe", "models.backbones_3d.spconv_backbone"])
    b2d = sys.modules["pcdet_ref.models.backbones_2d"].BaseBEVBackbone
    names = ['car', 'truck', 'construction_vehicle', 'bus', 'trailer', 'barrier', 'motorcycle', 'bicycle', 'pedestrian',
             'traffic_cone']
    out = {'head_n': shapes(n_head)}
    settings = {
        # a 44 x 36 pillar grid, two levels of the 2D backbone: an 11 x 9 map at stride 4
        'PointPillar': ('nuscenes_models/cbgs_pp_multihead.yaml',
                        {'LAYER_NUMS': [1, 1], 'LAYER_STRIDES': [2, 2], 'NUM_FILTERS': [64, 128], 'UPSAMPLE_STRIDES': [0.5, 1],
                         'NUM_UPSAMPLE_FILTERS': [128, 128]},
                        {'point_cloud_range': [0, -3.6, -5.0, 8.8, 3.6, 3.0], 'voxel_size': [0.2, 0.2, 8.0]}, [44, 36, 1]),
        # 16 x 16 x 40 cells, the smallest grid of the 8x backbone: a 2 x 2 map at stride 8
        'SECONDNet': ('nuscenes_models/cbgs_second_multihead.yaml', {'LAYER_NUMS': [1, 1]},
                      {'point_cloud_range': [0, -0.8, -5.0, 1.6, 0.8, 3.0], 'voxel_size': [0.1, 0.1, 0.2]}, [16, 16, 40]),
    }
    for name, (yaml_name, cut, dataset, grid) in settings.items():
        model_cfg = model_yaml(root, yaml_name)['MODEL']
        model_cfg['BACKBONE_2D'].update(cut)
        dataset = dict(dataset, class_names=names, num_point_features=5)
        cfg = to_attr(model_cfg)
        pcr, vs = np.array(dataset['point_cloud_range'], np.float64), np.array(dataset['voxel_size'], np.float64)
        if name == 'PointPillar':
            vfe = pvfe.PillarVFE(model_cfg=cfg.VFE, num_point_features=5, voxel_size=vs, point_cloud_range=pcr, grid_size=np.array(grid))
            front = shapes(vfe, "vfe.")
        else:
            front = shapes(getattr(b3d, cfg.BACKBONE_3D.NAME)(cfg.BACKBONE_3D, 5, np.array(grid)), "backbone_3d.")
        bev = b2d(cfg.BACKBONE_2D, input_channels=cfg.MAP_TO_BEV.NUM_BEV_FEATURES)
        head = multi.AnchorHeadMulti(model_cfg=cfg.DENSE_HEAD, input_channels=bev.num_bev_features, num_class=10, class_names=names,
                                     grid_size=np.array(grid), point_cloud_range=pcr, predict_boxes_when_training=False)
        out[name] = {'config': {'MODEL': model_cfg, 'dataset': dataset, 'grid_size': grid},
                     'state_dict': front + shapes(bev, "backbone_2d.") + shapes(head, "dense_head.")}
    write_state_dict("anchor_head_coded_state_dicts.json", out)


def main():
    root = reference_root()
    oracle.build()
    multi, template, box_utils = base.load_reference(root)
    rng = np.random.default_rng(20261021)
    torch.manual_seed(19)
    out = {'configs': np.array(json.dumps({'point_cloud_range': PCR, 'voxel_size': VOXEL, 'class_names': CLASS_NAMES,
                                           'heads': CONFIGS, 'post': POST, 'layout': LAYOUT}))}
    n_head = None
    for name, cfg in CONFIGS.items():
        code, sincos, extra = LAYOUT[name]
        C = len(CLASS_NAMES[name])
        head = make_head(multi, name)
        assert head.box_coder.code_size == code and head.anchors[0].shape[-1] == code
        n_head = head if name == 'n' else n_head
        out['keys_' + name] = np.array(list(head.state_dict().keys()), dtype='<U80')
        out['shapes_' + name] = np.array(json.dumps([list(v.shape) for v in head.state_dict().values()]))
        plain = seven(head)
        for c, a in enumerate(plain.anchors):
            out['%s_anchors_%d' % (name, c)] = a.numpy().copy()
        table, class_rows = base.table_of(plain)
        out[name + '_table'], out[name + '_class_rows'] = table, np.array(class_rows, np.int64)
        rows, cols = base.head_layout(cfg, class_rows)
        N = table.shape[0]
        assert N % 64 and N % 256 and all(r % 64 for r in class_rows)
        rich, only = base.scenes(cfg, plain, box_utils)
        rich, only = with_velocities(rich, extra, 0), with_velocities(only, extra, 1)
        assert rich.shape == (M, 8 + extra) and np.array_equal(rich[0], rich[1]) and not rich[6].any() and not rich[-3:].any()
        empty = np.zeros_like(rich)
        batches = (('x', np.stack([rich, only])), ('y', np.stack([empty, only])), ('z', np.stack([empty, empty])))
        ious = base.check_inputs(cfg, plain, as_eight(batches[0][1]), box_utils)
        for c, iou in enumerate(ious):
            out['%sx_iou_%d' % (name, c)] = iou
        first = base.run_batch({}, 'tmp_', cfg, head, batches[0][1], None, table, rows, cols)
        first_labels, first_targets = first['box_cls_labels'].numpy(), first['box_reg_targets'].numpy()
        assert first_targets.shape == (B, N, code)
        positives = np.nonzero(first_labels > 0)
        preds, kink = predictions(rng, name, cfg, table, positives, first_targets)
        for key, v in zip(('cls', 'box', 'dir'), preds):
            if v is not None:
                out['%s_%s_preds' % (name, key)] = v.astype(np.float16)
                assert np.array_equal(v.astype(np.float16).astype(np.float32), v)
        if sincos:
            out[name + '_min_hypot'] = np.float64(min_hypot(preds[1], table))
            assert out[name + '_min_hypot'] >= MIN_HYPOT
            print(name, 'min hypot', out[name + '_min_hypot'])
        for tag, gt in batches:
            base.check_inputs(cfg, plain, as_eight(gt), box_utils)
            base.run_batch(out, name + tag + '_', cfg, head, gt, preds, table, rows, cols)
            lab = out[name + tag + '_box_cls_labels']
            print(name, tag, 'positives', (lab > 0).sum(axis=1), 'ignored', (lab < 0).sum(axis=1), 'losses', out[name + tag + '_losses'])
            assert np.isfinite(out[name + tag + '_losses']).all()
            for k in out:
                if k.startswith(name + tag + '_g_'):
                    assert np.isfinite(out[k]).all(), k
        base.decode_case(out, name, cfg, head, preds, table, rows)
        assert out[name + '_batch_box_preds'].shape == (B, N, 7 + extra)
        # the cases the rich scene is there for, as in make_anchor_head_multi_golden.py
        lab = out[name + 'x_box_cls_labels'][0]
        first_row = np.concatenate([[0], np.cumsum(class_rows)])
        iou_all = np.zeros((N, M), np.float32)
        for c, iou in enumerate(ious):
            iou_all[first_row[c]:first_row[c + 1]] = iou
        row_label = np.repeat(np.arange(1, C + 1), class_rows)
        sq = iou_all[:, 2] * (row_label == base.RICH['square'][0])
        assert (sq == sq.max()).sum() >= 2 and sq.max() > 0 and (lab[sq == sq.max()] > 0).all(), "a tie on the square box"
        assert iou_all[:, 4].max() == 0, "a box that overlaps no anchor"
        small = iou_all[:, 3] * (row_label == base.RICH['small'][0])
        thr = cfg['ANCHOR_GENERATOR_CONFIG'][base.RICH['small'][0] - 1]['unmatched_threshold']
        assert 0 < small.max() < thr and (lab[small == small.max()] > 0).all(), "a forced positive below the unmatched threshold"
        assert (out[name + 'z_box_cls_labels'] == 0).all() and (lab < 0).any()
        only_lab = out[name + 'x_box_cls_labels'][1]
        assert (only_lab[:class_rows[0]] > 0).any() and (only_lab[class_rows[0]:] == 0).all(), "the other heads are background"
        if extra:
            t = out[name + 'x_box_reg_targets'][out[name + 'x_box_cls_labels'] > 0][:, code - extra:]
            nan = np.isnan(t)
            assert nan.any(axis=1).sum() >= 2 and (nan.sum(axis=1) == 1).any() and nan.all(axis=1).any(), "the NaN velocities"
            assert not np.isnan(out[name + 'x_box_reg_targets'][..., :code - extra]).any()
        if kink is not None:
            assert out['nx_box_cls_labels'][kink[:2]] > 0 and preds[1][kink] == out['nx_box_reg_targets'][kink]
            assert out['nx_g_box_%d' % 0].shape[-1] == code
            out['n_kink'] = np.array(kink, np.int64)
        if name == 'n':
            post_case(out, name, head, template, table, rows, cols, batches[0][1], rng)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 1 << 20
    state_dicts(root, multi, n_head)


if __name__ == "__main__":
    main()
