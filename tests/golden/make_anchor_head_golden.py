#!/usr/bin/env python
"""Generates tests/golden/anchor_head.npz: the REFERENCE's anchor head and hard-voxel PillarVFE run on synthetic batches on
CPU tensors -- AnchorGenerator, AxisAlignedTargetAssigner.assign_targets with the IoU matrices of the first scene,
AnchorHeadTemplate.get_loss with its gradients, generate_predicted_boxes, PillarVFE with its PFN input rows, and the
state-dict keys of AnchorHeadSingle and PillarVFE.

The reference's own anchor_head_template.py, anchor_head_single.py, anchor_generator.py, axis_aligned_target_assigner.py,
pillar_vfe.py, loss_utils.py, box_coder_utils.py, box_utils.py and common_utils.py are loaded as pcdet_ref.* with their
package imports stubbed (reference_loader.py).

Two configurations, B = 2, M = 12:
  a  range [0, -8, -3, 12.8, 8, 1], voxels of 0.2 m, stride 2: a 32 x 40 map; the three KITTI anchor classes with the yaml's
     sizes, rotations and thresholds, align_center False, direction classifier on: 7680 anchors a scene;
  b  one class, num_class 1, two anchor sizes and two bottom heights, align_center True, a 25 x 19 map: 3800 anchors a scene
     (a multiple of neither 64 nor 256), no direction classifier, non-uniform code_weights.
Three batches each: x = [rich scene, one class only], y = [empty, one class only], z = [empty, empty] (num_pos == 0).
The rich scene holds two identical boxes, a square box centred on an anchor location of the table (both rotations tie
for its column maximum), a small box between locations whose best anchor lies below unmatched_threshold (a forced
positive that survives the background write), a box that overlaps no anchor, a heading past pi / 4, an interior zero row
and trailing zero rows.

To keep the file small the predictions take few distinct values: class logits are multiples of 1/4, box codes are zero
around -6 (the head's initial bias is -4.6), box codes are zero
except at a fifth of the anchors and at every positive (multiples of 1/64), direction logits multiples of 1/8.

The maker asserts on its own inputs: no |r - pi/4| below 1e-4; no direction offset within 1e-4 of a bin edge (targets and
decoding); no row_max within 1e-6 of a threshold; no two top direction logits equal.

Run with the reference checkout:  python tests/golden/make_anchor_head_golden.py /path/to/reference
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from reference_loader import ANCHOR_HEAD, MODEL_UTILS, cpu_torch, extension_stubs, load, reference_root  # noqa: E402
from pdanet_amd.config import to_attr  # noqa: E402

OUT = os.path.join(HERE, "anchor_head.npz")
B, M = 2, 12
AHS = PVFE = BOX_UTILS = None       # the reference's anchor_head_single, pillar_vfe and box_utils, once load_reference has run


def load_reference(root):
    global AHS, PVFE, BOX_UTILS
    cpu_torch()
    needed = load(root, "pcdet_ref", MODEL_UTILS + ANCHOR_HEAD + ["models.backbones_3d.vfe.vfe_template"],
                  stubs=extension_stubs())
    BOX_UTILS = needed[MODEL_UTILS.index("utils.box_utils")]
    AHS, PVFE = load(root, "pcdet_ref", ["models.dense_heads.anchor_head_single", "models.backbones_3d.vfe.pillar_vfe"])


TARGET = {'NAME': 'AxisAlignedTargetAssigner', 'POS_FRACTION': -1.0, 'SAMPLE_SIZE': 512, 'NORM_BY_NUM_EXAMPLES': False,
          'MATCH_HEIGHT': False, 'BOX_CODER': 'ResidualCoder'}
CONFIGS = {
    # kitti_models/pointpillar.yaml DENSE_HEAD on a 32 x 40 map
    'a': {
        'point_cloud_range': [0, -8, -3, 12.8, 8, 1], 'voxel_size': [0.2, 0.2, 4], 'class_names': ['Car', 'Pedestrian', 'Cyclist'],
        'num_class': 3,
        'head': {
            'CLASS_AGNOSTIC': False, 'USE_DIRECTION_CLASSIFIER': True, 'DIR_OFFSET': 0.78539, 'DIR_LIMIT_OFFSET': 0.0,
            'NUM_DIR_BINS': 2,
            'ANCHOR_GENERATOR_CONFIG': [
                {'class_name': 'Car', 'anchor_sizes': [[3.9, 1.6, 1.56]], 'anchor_rotations': [0, 1.57],
                 'anchor_bottom_heights': [-1.78], 'align_center': False, 'feature_map_stride': 2, 'matched_threshold': 0.6,
                 'unmatched_threshold': 0.45},
                {'class_name': 'Pedestrian', 'anchor_sizes': [[0.8, 0.6, 1.73]], 'anchor_rotations': [0, 1.57],
                 'anchor_bottom_heights': [-0.6], 'align_center': False, 'feature_map_stride': 2, 'matched_threshold': 0.5,
                 'unmatched_threshold': 0.35},
                {'class_name': 'Cyclist', 'anchor_sizes': [[1.76, 0.6, 1.73]], 'anchor_rotations': [0, 1.57],
                 'anchor_bottom_heights': [-0.6], 'align_center': False, 'feature_map_stride': 2, 'matched_threshold': 0.5,
                 'unmatched_threshold': 0.35}],
            'TARGET_ASSIGNER_CONFIG': TARGET,
            'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0, 'dir_weight': 0.2,
                                             'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}}},
    # one class, two sizes, two bottom heights, centred anchors, no direction classifier
    'b': {
        'point_cloud_range': [0, -3.8, -3, 10.0, 3.8, 1], 'voxel_size': [0.4, 0.4, 4], 'class_names': ['Car'], 'num_class': 1,
        'head': {
            'CLASS_AGNOSTIC': False,
            'ANCHOR_GENERATOR_CONFIG': [
                {'class_name': 'Car', 'anchor_sizes': [[3.9, 1.6, 1.56], [2.4, 1.2, 1.4]], 'anchor_rotations': [0, 1.57],
                 'anchor_bottom_heights': [-1.78, -1.0], 'align_center': True, 'feature_map_stride': 1,
                 'matched_threshold': 0.6, 'unmatched_threshold': 0.45}],
            'TARGET_ASSIGNER_CONFIG': TARGET,
            'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0, 'dir_weight': 0.2,
                                             'code_weights': [1.0, 1.0, 0.5, 1.0, 1.0, 2.0, 0.75]}}}},
}
# per configuration: the class (1-based label) and side of the square box, the class and size of the small box, the class of
# the box with a heading past pi / 4, the class of the last box, and the map cell (y, x) of the square / near the small box
RICH = {'a': {'square': (2, 0.7, (12, 20)), 'small': (2, (0.3, 0.3, 1.6), (25, 9)), 'turned': 3, 'last': 3},
        'b': {'square': (1, 2.0, (9, 12)), 'small': (1, (0.6, 0.5, 1.4), (15, 4)), 'turned': 1, 'last': 1}}


def make_head(cfg):
    pcr, vs = np.array(cfg['point_cloud_range'], np.float64), np.array(cfg['voxel_size'], np.float64)
    grid = np.round((pcr[3:] - pcr[:3]) / vs).astype(np.int64)
    return AHS.AnchorHeadSingle(model_cfg=to_attr(cfg['head']), input_channels=16, num_class=cfg['num_class'],
                                class_names=cfg['class_names'], grid_size=grid, point_cloud_range=pcr,
                                predict_boxes_when_training=False)


def table_of(head):
    flat = [a.reshape(*a.shape[:3], -1, 7) for a in head.anchors]
    return torch.cat(flat, dim=-2).reshape(-1, 7).numpy().copy(), [f.shape[3] for f in flat]


def scenes(name, cfg, head):
    r = RICH[name]
    pcr = cfg['point_cloud_range']
    sizes = {c['class_name']: c['anchor_sizes'][0] for c in cfg['head']['ANCHOR_GENERATOR_CONFIG']}
    size_of = lambda label: np.array(sizes[cfg['class_names'][label - 1]])
    car = size_of(1)
    rich = np.zeros((M, 8), np.float64)
    rich[0] = rich[1] = [pcr[0] + 5.03, pcr[1] + 5.02, -1.0, car[0] * 1.05, car[1] * 0.95, car[2], 0.1, 1]
    label, side, (iy, ix) = r['square']
    cls_idx = [c['class_name'] for c in cfg['head']['ANCHOR_GENERATOR_CONFIG']].index(cfg['class_names'][label - 1])
    # an anchor location of the table at which the float32 IoUs of the two rotations are bit-equal (the corners are rounded,
    # so this holds at some locations only): scan from the given cell on
    anc = head.anchors[cls_idx]
    found = None
    for cell in range(iy * anc.shape[2] + ix, anc.shape[1] * anc.shape[2]):
        cy, cx = divmod(cell, anc.shape[2])
        loc = anc[0, cy, cx, 0, 0].numpy().astype(np.float64)
        row = np.array([[loc[0], loc[1], loc[2], side, side, size_of(label)[2], 0.0]], np.float32)
        pair = BOX_UTILS.boxes3d_nearest_bev_iou(anc[0, cy, cx, 0].reshape(-1, 7), torch.from_numpy(row)).numpy()[:, 0]
        if pair[0] == pair[1] and pair[0] > 0:
            found = row[0]
            break
    assert found is not None, "no location where both rotations tie"
    rich[2, :7], rich[2, 7] = found, label
    label, dims, (iy, ix) = r['small']
    cls_idx = [c['class_name'] for c in cfg['head']['ANCHOR_GENERATOR_CONFIG']].index(cfg['class_names'][label - 1])
    loc = head.anchors[cls_idx][0, iy, ix, 0, 0].numpy().astype(np.float64)
    rich[3] = [loc[0] + 0.13, loc[1] + 0.17, loc[2], dims[0], dims[1], dims[2], 0.2, label]
    rich[4] = [pcr[3] + 27.0, 0.5, -1.0, 1.8, 0.6, 1.7, 0.3, r['last']]                  # overlaps no anchor
    t = size_of(r['turned'])
    rich[5] = [pcr[0] + 9.1, pcr[1] + 2.3, -0.8, t[0] * 0.97, t[1] * 1.1, t[2], 1.3, r['turned']]      # a heading past pi / 4
    # row 6 stays zero
    rich[7] = [pcr[0] + 2.4, pcr[1] + 1.9, -1.1, car[0] * 0.9, car[1] * 1.02, car[2] * 1.1, -2.0, 1]
    t = size_of(r['last'])
    rich[8] = [pcr[0] + 7.7, pcr[3 + 1] - 1.3, -0.7, t[0] * 1.08, t[1] * 0.93, t[2] * 0.95, 0.35, r['last']]
    only = np.zeros((M, 8), np.float64)
    only[0] = [pcr[0] + 3.3, pcr[1] + 3.1, -0.9, car[0], car[1] * 1.1, car[2], 0.05, 1]
    only[2] = [pcr[0] + 8.6, pcr[1] + 4.4, -1.2, car[0] * 0.92, car[1], car[2] * 0.9, 1.5, 1]
    only[3] = [pcr[0] + 6.2, pcr[4] - 1.1, -1.0, car[0] * 1.1, car[1] * 0.9, car[2], -0.4, 1]
    return rich.astype(np.float32), only.astype(np.float32)


def check_inputs(cfg, head, gt):
    """The conditions on the inputs, with the reference alone.  Returns the per-class IoU matrices of scene 0."""
    def away(boxes):
        ry = boxes[:, 6].astype(np.float64)
        rr = np.abs(ry - np.floor(ry / np.pi + 0.5) * np.pi)
        assert (np.abs(rr - np.pi / 4) >= 1e-4).all(), "a heading next to pi / 4"
    ious = []
    for s in range(gt.shape[0]):
        live = gt[s][np.abs(gt[s]).sum(-1) > 0]
        away(live)
        for c, (anchors, acfg) in enumerate(zip(head.anchors, cfg['head']['ANCHOR_GENERATOR_CONFIG'])):
            a = anchors.reshape(-1, 7)
            away(a.numpy())
            iou = BOX_UTILS.boxes3d_nearest_bev_iou(a, torch.from_numpy(gt[s, :, :7].copy())).numpy()
            if s == 0:
                ious.append(iou)
            label = cfg['class_names'].index(acfg['class_name']) + 1
            mine = iou[:, gt[s, :, 7] == label]
            if mine.shape[1]:
                row_max = mine.max(axis=1).astype(np.float64)
                for thr in (acfg['matched_threshold'], acfg['unmatched_threshold']):
                    assert (np.abs(row_max - thr) >= 1e-6).all(), "a row maximum next to a threshold"
    return ious


def predictions(rng, cfg, N, positives):
    nc = cfg['num_class']
    # logits around the head's initial bias, so that the loss of an empty scene (normaliser 1) stays of order one
    cls = np.clip(np.round((rng.standard_normal((B, N, nc)) - 6.0) * 4) / 4, -9, -2.5).astype(np.float32)
    cls[positives[0][:4], positives[1][:4], 0] = [2.5, -6.0, 0.25, -1.5]
    box = np.round(rng.standard_normal((B, N, 7)) * 0.3 * 64) / 64
    keep = rng.random((B, N)) < 0.2
    keep[positives] = True
    box = (box * keep[..., None]).astype(np.float32)
    d = None
    if cfg['head'].get('USE_DIRECTION_CLASSIFIER'):
        bins = cfg['head']['NUM_DIR_BINS']
        d = np.round(rng.standard_normal((B, N, bins)) * 8) / 8
        d[..., 1] = d[..., 0] + rng.choice([-1.5, -0.5, -0.125, 0.125, 0.75, 2.0], size=(B, N))
        d = d.astype(np.float32)
        top = np.sort(d, axis=-1)
        assert (top[..., -1] > top[..., -2]).all(), "two top direction logits equal"
    return cls, box, d


def run_batch(out, p, cfg, head, gt, preds, table, counts):
    H, W = head.anchors[0].shape[1:3]
    targets = head.assign_targets(torch.from_numpy(gt.copy()))
    labels = targets['box_cls_labels'].numpy().copy()
    out[p + 'gt_boxes'] = gt
    out[p + 'box_cls_labels'] = labels.astype(np.int32)
    out[p + 'box_reg_targets'] = targets['box_reg_targets'].numpy().copy()
    out[p + 'reg_weights'] = targets['reg_weights'].numpy().copy()
    if preds is None:
        return targets
    cls, box, d = preds
    N = table.shape[0]
    A = N // (H * W)
    leaves = {'cls_preds': torch.from_numpy(cls.reshape(B, H, W, -1).copy()).requires_grad_(True),
              'box_preds': torch.from_numpy(box.reshape(B, H, W, -1).copy()).requires_grad_(True)}
    if d is not None:
        leaves['dir_cls_preds'] = torch.from_numpy(d.reshape(B, H, W, -1).copy()).requires_grad_(True)
    head.num_anchors_per_location = A
    head.forward_ret_dict = dict(leaves, box_cls_labels=targets['box_cls_labels'].clone(),
                                 box_reg_targets=targets['box_reg_targets'].clone(), reg_weights=targets['reg_weights'].clone())
    loss, tb = head.get_loss()
    loss.backward()
    out[p + 'losses'] = np.array([tb['rpn_loss_cls'], tb['rpn_loss_loc'], tb.get('rpn_loss_dir', 0.0), tb['rpn_loss']], np.float64)
    for k, v in leaves.items():
        out[p + 'g_' + k] = v.grad.numpy().reshape(B, N, -1).copy()
    if d is not None:      # the direction offsets of the positives against the bin edges
        pos = labels > 0
        rot = (targets['box_reg_targets'].numpy()[..., 6].astype(np.float64) + table[None, :, 6])[pos] - cfg['head']['DIR_OFFSET']
        q = (rot - np.floor(rot / (2 * np.pi)) * 2 * np.pi) / (2 * np.pi / cfg['head']['NUM_DIR_BINS'])
        assert (np.abs(q - np.round(q)) >= 1e-4).all(), "a direction offset next to a bin edge"
    return targets


def decode_case(out, name, cfg, head, preds, table):
    H, W = head.anchors[0].shape[1:3]
    cls, box, d = preds
    with torch.no_grad():
        bc, bb = head.generate_predicted_boxes(
            B, torch.from_numpy(cls.reshape(B, H, W, -1).copy()), torch.from_numpy(box.reshape(B, H, W, -1).copy()),
            None if d is None else torch.from_numpy(d.reshape(B, H, W, -1).copy()))
    assert np.array_equal(bc.numpy(), cls)                      # batch_cls_preds is the input viewed (B, N, num_class)
    out[name + '_batch_box_preds'] = bb.numpy().copy()
    if d is not None:
        period = 2 * np.pi / cfg['head']['NUM_DIR_BINS']
        rg = box[..., 6].astype(np.float64) + table[None, :, 6]
        q = (rg - cfg['head']['DIR_OFFSET']) / period + cfg['head']['DIR_LIMIT_OFFSET']
        assert (np.abs(q - np.round(q)) >= 1e-4).all(), "a decoded heading next to a bin edge"


def vfe_case(out, rng):
    """About 200 voxels of P = 32 rows and C = 4 columns on configuration a's grid, among them voxels with 1 and with 32
    points; PillarVFE with (USE_ABSLOTE_XYZ True, WITH_DISTANCE False) and (False, True): its PFN input rows and its output
    in train and eval mode, with the BatchNorm parameters and running statistics drawn at random."""
    cfg = CONFIGS['a']
    pcr, vs = np.array(cfg['point_cloud_range'], np.float64), np.array(cfg['voxel_size'], np.float64)
    V, P, C = 203, 32, 4
    nx, ny = 64, 80
    cells = np.sort(rng.permutation(2 * ny * nx)[:V])
    coords = np.zeros((V, 4), np.int32)
    coords[:, 0], coords[:, 2], coords[:, 3] = cells // (ny * nx), (cells % (ny * nx)) // nx, cells % nx
    num = np.minimum(1 + rng.geometric(0.3, size=V), P).astype(np.int32)
    num[0], num[1], num[2], num[3] = 1, 32, 31, 2
    voxels = np.zeros((V, P, C), np.float32)
    for v in range(V):
        lo = pcr[:3] + vs * np.array([coords[v, 3], coords[v, 2], coords[v, 1]])
        n = num[v]
        voxels[v, :n, :3] = lo + rng.random((n, 3)) * vs
        voxels[v, :n, 3] = np.round(rng.random(n) * 256) / 256
    out['v_voxels'], out['v_coords'], out['v_num_points'] = voxels, coords, num
    for tag, absolute, dist, filters in (('p', True, False, [8, 16]), ('q', False, True, [16])):
        mcfg = {'USE_NORM': True, 'WITH_DISTANCE': dist, 'USE_ABSLOTE_XYZ': absolute, 'NUM_FILTERS': filters}
        torch.manual_seed(5)
        vfe = PVFE.PillarVFE(to_attr(mcfg), num_point_features=C, voxel_size=vs, point_cloud_range=pcr)
        sd = vfe.state_dict()
        for k in sd:
            if k.endswith('norm.weight') or k.endswith('running_var'):
                sd[k] = torch.rand_like(sd[k]) + 0.5
            elif k.endswith('norm.bias') or k.endswith('running_mean'):
                sd[k] = torch.randn_like(sd[k]) * 0.3
        vfe.load_state_dict(sd)
        out['v%s_cfg' % tag] = np.array(json.dumps(mcfg))
        out['v%s_keys' % tag] = np.array(list(sd.keys()), dtype='<U80')
        for k, v in sd.items():
            out['v%s_sd_%s' % (tag, k)] = v.numpy().copy()
        seen = []
        hook = vfe.pfn_layers[0].register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().numpy().copy()))
        batch = lambda: {'voxels': torch.from_numpy(voxels.copy()), 'voxel_num_points': torch.from_numpy(num.copy()),
                         'voxel_coords': torch.from_numpy(coords.copy())}
        with torch.no_grad():
            vfe.eval()
            out['v%s_out_eval' % tag] = vfe(batch())['pillar_features'].numpy().copy()
            vfe.train()
            out['v%s_out_train' % tag] = vfe(batch())['pillar_features'].numpy().copy()
        hook.remove()
        out['v%s_features' % tag] = seen[0]
        assert np.array_equal(seen[0], seen[1]) and not seen[0][0, 1:].any() and seen[0][1, 31].any()


def main():
    load_reference(reference_root())
    rng = np.random.default_rng(20261019)
    torch.manual_seed(13)
    out = {'configs': np.array(json.dumps(CONFIGS))}
    for name, cfg in CONFIGS.items():
        head = make_head(cfg)
        out['keys_%s' % name] = np.array(list(head.state_dict().keys()), dtype='<U80')
        for c, a in enumerate(head.anchors):
            out['%s_anchors_%d' % (name, c)] = a.numpy().copy()
        table, counts = table_of(head)
        out['%s_table' % name], out['%s_counts' % name] = table, np.array(counts, np.int64)
        N = table.shape[0]
        rich, only = scenes(name, cfg, head)
        empty = np.zeros_like(rich)
        batches = (('x', np.stack([rich, only])), ('y', np.stack([empty, only])), ('z', np.stack([empty, empty])))
        ious = check_inputs(cfg, head, batches[0][1])
        for c, iou in enumerate(ious):
            out['%sx_iou_%d' % (name, c)] = iou
        first = run_batch(out, 'tmp_', cfg, head, batches[0][1], None, table, counts)
        for k in [k for k in out if k.startswith('tmp_')]:
            del out[k]
        positives = np.nonzero(first['box_cls_labels'].numpy() > 0)
        preds = predictions(rng, cfg, N, positives)
        out[name + '_cls_preds'], out[name + '_box_preds'] = preds[0].astype(np.float16), preds[1].astype(np.float16)
        assert np.array_equal(out[name + '_cls_preds'].astype(np.float32), preds[0])
        assert np.array_equal(out[name + '_box_preds'].astype(np.float32), preds[1])
        if preds[2] is not None:
            out[name + '_dir_cls_preds'] = preds[2].astype(np.float16)
            assert np.array_equal(out[name + '_dir_cls_preds'].astype(np.float32), preds[2])
        for tag, gt in batches:
            check_inputs(cfg, head, gt)
            run_batch(out, name + tag + '_', cfg, head, gt, preds, table, counts)
            lab = out[name + tag + '_box_cls_labels']
            print(name, tag, 'positives', (lab > 0).sum(axis=1), 'ignored', (lab < 0).sum(axis=1), 'losses', out[name + tag + '_losses'])
        decode_case(out, name, cfg, head, preds, table)
        # the cases the rich scene is there for
        lab = out[name + 'x_box_cls_labels'][0]
        iou_all = np.zeros((N, M), np.float32)
        slots = sum(counts)
        slot_class = np.concatenate([np.full(k, c) for c, k in enumerate(counts)])
        for c, iou in enumerate(ious):
            rows = np.nonzero(slot_class[np.arange(N) % slots] == c)[0]
            iou_all[rows] = iou
        sq_label = RICH[name]['square'][0]
        sq_col = iou_all[:, 2] * (lab == sq_label)
        assert (sq_col == sq_col.max()).sum() >= 2 and sq_col.max() > 0, "both rotations tie on the square box"
        assert iou_all[:, 4].max() == 0, "a box that overlaps no anchor"
        acfg = cfg['head']['ANCHOR_GENERATOR_CONFIG']
        row_label = np.array([cfg['class_names'].index(c['class_name']) + 1 for c in acfg])[slot_class[np.arange(N) % slots]]
        small = iou_all[:, 3] * (row_label == RICH[name]['small'][0])
        thr = [c for c in acfg if c['class_name'] == cfg['class_names'][RICH[name]['small'][0] - 1]][0]['unmatched_threshold']
        assert 0 < small.max() < thr and (lab[small == small.max()] > 0).all(), "a forced positive below the unmatched threshold"
        assert (out[name + 'z_box_cls_labels'] == 0).all()
    vfe_case(out, rng)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 1 << 20


if __name__ == "__main__":
    main()
