#!/usr/bin/env python
"""Times the dense head of nuscenes_models/cbgs_pp_multihead.yaml at the yaml's shape: 4 scenes, a 128 x 128 map, ten classes of
two rotations = 327 680 anchors a scene in six heads, 10-wide codes (sin-cos heading, two velocity columns), WeightedL1Loss,
SCORE_THRESH 0.1, NMS_PRE_MAXSIZE / NMS_POST_MAXSIZE 1000 / 83, on synthetic tensors.  The head's settings are the yaml's
DENSE_HEAD and POST_PROCESSING blocks as tests/golden/anchor_head_coded_state_dicts.json records them.

  train   targets + loss + backward.  device: pda_anchor_multi_assign_targets_coded, pda_anchor_multi_loss_coded and the
          gradient scaling (csrc/anchor_head.hip).  torch: the reference's order of work on the same card -- per scene the
          trailing-zero trim (host reads), per anchor class the anchors x gts IoU matrix, two argmaxes, nonzero() compactions,
          boolean-mask writes and ResidualCoder.encode_torch against the zero-padded anchors; then per head the one-hot slice,
          the focal loss with pos / neg weights, WeightedL1Loss, and autograd's backward (without the reference's .item() reads).
  post    post-processing with MULTI_CLASSES_NMS on 9-column boxes.  device: model_nms_utils.post_processing, no host read.
          torch: the reference's loop over scenes, heads and classes (benchmarks/second_multihead.py post_torch).

Timing as in benchmarks/second_multihead.py: the sides alternate inside one process, wall-clock milliseconds between two device
synchronisations per call, median, minimum, maximum.  The labels of the two target assignments and the detections of the two
post-processings are compared before anything is timed.  A measurement, not a gate: prints one JSON line.

    python benchmarks/nuscenes_multihead.py [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "benchmarks")]

from pdanet_amd import anchor_head_coded as ahc, loss_utils, model_nms_utils      # noqa: E402
from pdanet_amd.config import to_attr                                             # noqa: E402
from anchor_head_bench import nearest_bev_iou                                     # noqa: E402
from second_multihead import post_torch, timed_alternating                        # noqa: E402

PCR, VOXEL = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], [0.2, 0.2, 8.0]


def settings():
    with open(os.path.join(ROOT, "tests", "golden", "anchor_head_coded_state_dicts.json")) as f:
        cfg = json.load(f)['PointPillar']['config']
    return cfg['MODEL']['DENSE_HEAD'], cfg['MODEL']['POST_PROCESSING'], cfg['dataset']['class_names']


def synth(rng, B, m, n_live, gen):
    """(B, m, 10) gt boxes: the classes' anchor sizes jittered, velocities (a fifth of them NaN), the 1-based label."""
    gt = np.zeros((B, m, 10), np.float32)
    for b in range(B):
        k = n_live[b % len(n_live)]
        cls = rng.integers(0, len(gen), k)
        gt[b, :k, 0], gt[b, :k, 1] = rng.uniform(PCR[0] + 2, PCR[3] - 2, k), rng.uniform(PCR[1] + 2, PCR[4] - 2, k)
        gt[b, :k, 2] = rng.uniform(-1.5, 0.0, k)
        gt[b, :k, 3:6] = np.array([gen[c]['anchor_sizes'][0] for c in cls]) * rng.uniform(0.85, 1.15, (k, 3))
        gt[b, :k, 6] = rng.uniform(-np.pi, np.pi, k)
        vel = rng.uniform(-5, 5, (k, 2))
        vel[rng.random(k) < 0.2] = np.nan
        gt[b, :k, 7:9], gt[b, :k, 9] = vel, cls + 1
    return gt


def targets_torch(class_tables, gt_all, coder, gen):
    """The reference's order of work with use_multihead: per scene, per anchor class over its class-major rows; the anchors
    carry the reference's zero columns."""
    out_l, out_t = [], []
    for k in range(gt_all.shape[0]):
        cur = gt_all[k]
        cnt = cur.shape[0] - 1
        while cnt > 0 and cur[cnt, :7].sum() == 0:              # the reference's trim: one host read per step
            cnt -= 1
        cur = cur[:cnt + 1]
        classes = cur[:, -1].int()
        labels_k, targets_k = [], []
        for c, anc in enumerate(class_tables):
            mask = classes == c + 1
            gts, gcls = cur[mask, :-1], classes[mask]
            n = anc.shape[0]
            labels = torch.full((n,), -1, dtype=torch.int32, device=anc.device)
            targets = anc.new_zeros((n, coder.code_size))
            if gts.shape[0] > 0:
                iou = nearest_bev_iou(anc[:, :7], gts[:, :7])
                a2g = iou.argmax(dim=1)
                a2g_max = iou[torch.arange(n, device=anc.device), a2g]
                g2a = iou.argmax(dim=0)
                g2a_max = iou[g2a, torch.arange(gts.shape[0], device=anc.device)]
                g2a_max[g2a_max == 0] = -1
                forced = (iou == g2a_max).nonzero()[:, 0]
                force_gt = a2g[forced]
                labels[forced] = gcls[force_gt]
                pos = a2g_max >= gen[c]['matched_threshold']
                labels[pos] = gcls[a2g[pos]]
                labels[(a2g_max < gen[c]['unmatched_threshold']).nonzero()[:, 0]] = 0
                labels[forced] = gcls[force_gt]
                fg = (labels > 0).nonzero()[:, 0]
                targets[fg] = coder.encode_torch(gts[a2g[fg]], anc[fg])
            else:
                labels[:] = 0
            labels_k.append(labels)
            targets_k.append(targets)
        out_l.append(torch.cat(labels_k))
        out_t.append(torch.cat(targets_k))
    return torch.stack(out_l), torch.stack(out_t)


def loss_torch(cls_preds, box_preds, labels, targets, cols, weights, funcs):
    """get_cls_layer_loss + get_box_reg_layer_loss of anchor_head_multi.py for a separate multihead without a direction
    classifier."""
    B, N = labels.shape
    num_class = sum(cols)
    cared, positives, negatives = labels >= 0, labels > 0, labels == 0
    norm = positives.sum(1, keepdim=True).float().clamp(min=1.0)
    cls_weights = (negatives * 1.0 * weights['neg_cls_weight'] + weights['pos_cls_weight'] * positives).float() / norm
    reg_weights = positives.float() / norm
    one_hot = torch.zeros(B, N, num_class + 1, dtype=cls_preds[0].dtype, device=labels.device)
    one_hot.scatter_(-1, (labels * cared.type_as(labels)).long().unsqueeze(-1), 1.0)
    one_hot = one_hot[..., 1:]
    start, c_idx, total = 0, 0, 0
    for cp, bp, k in zip(cls_preds, box_preds, cols):
        rows = slice(start, start + cp.shape[1])
        total = total + funcs[0](cp, one_hot[:, rows, c_idx:c_idx + k], weights=cls_weights[:, rows]).sum() / B * weights['cls_weight']
        total = total + funcs[1](bp, targets[:, rows], weights=reg_weights[:, rows]).sum() / B * weights['loc_weight']
        start += cp.shape[1]
        c_idx += k
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--max-gt", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/nuscenes_multihead.py needs the GPU: a CPU run gives no time")
    torch.cuda.set_device(0)
    B = args.batch
    head_cfg, post_cfg, names = settings()
    gen, weights = head_cfg['ANCHOR_GENERATOR_CONFIG'], head_cfg['LOSS_CONFIG']['LOSS_WEIGHTS']
    pcr, vs = np.array(PCR, np.float64), np.array(VOXEL, np.float64)
    grid = np.round((pcr[3:] - pcr[:3]) / vs).astype(np.int64)
    head = ahc.AnchorHeadMultiCoded(to_attr(head_cfg), 384, len(names), names, grid, pcr, predict_boxes_when_training=False).cuda()
    coder = head.box_coder
    rng = np.random.default_rng(0)
    gt = torch.from_numpy(synth(rng, B, args.max_gt, [args.max_gt, 30, 45, 12], gen)).cuda()
    table = head.anchor_table(gt.device)
    rows, cols = head.head_rows, [h.num_class for h in head.rpn_heads]
    per_class = table.shape[0] // len(gen)
    padded_table = torch.cat([table, table.new_zeros(table.shape[0], coder.code_size - 7)], dim=1)
    class_tables = [padded_table[c * per_class:(c + 1) * per_class] for c in range(len(gen))]
    dev = lambda x: torch.from_numpy(x.astype(np.float32)).cuda()
    cls_preds = [dev(rng.standard_normal((B, n, k)) - 4.6) for n, k in zip(rows, cols)]
    box_preds = [dev(rng.standard_normal((B, n, coder.code_size)) * 0.2) for n in rows]
    funcs = (loss_utils.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0),
             loss_utils.WeightedL1Loss(code_weights=weights['code_weights']).cuda())
    targets = head.assign_targets(gt)
    ref_labels, ref_targets = targets_torch(class_tables, gt, coder, gen)
    result = {"benchmark": "nuscenes_multihead", "batch": B, "anchors": int(table.shape[0]), "heads": rows, "code": coder.code_size,
              "max_gt": args.max_gt, "steps": args.steps, "warmup": args.warmup, "unit": "wall-clock ms per call (median, min, max)",
              "device": torch.cuda.get_device_name(0), "positives": targets['num_pos'].tolist(),
              "label_mismatches": int((ref_labels != targets['box_cls_labels']).sum())}

    def leaves():
        return [[t.detach().requires_grad_(True) for t in parts] for parts in (cls_preds, box_preds)]

    def train_device():
        c, b = leaves()
        head.forward_ret_dict = dict(head.assign_targets(gt), cls_preds=c, box_preds=b)
        loss = head.get_loss()[0]
        loss.backward()
        return loss

    def train_torch():
        c, b = leaves()
        labels, tg = targets_torch(class_tables, gt, coder, gen)
        loss = loss_torch(c, b, labels, tg, cols, weights, funcs)
        loss.backward()
        return loss

    result["loss_device_torch"] = [float(train_device().detach()), float(train_torch().detach())]
    result["train"] = timed_alternating({"device": train_device, "torch": train_torch}, args.steps, args.warmup)

    # post-processing: logits around the head's initial bias with a tail above the threshold, decoded boxes of small codes
    post_cls = [dev(rng.standard_normal((B, n, k)) * 1.6 - 4.6) for n, k in zip(rows, cols)]
    with torch.no_grad():
        _, boxes = head.generate_predicted_boxes(B, post_cls, box_preds, None)
    mapping = [h.head_label_indices for h in head.rpn_heads]
    batch = {'batch_size': B, 'batch_cls_preds': post_cls, 'batch_box_preds': boxes, 'cls_preds_normalized': False,
             'multihead_label_mapping': mapping}
    cfg = to_attr(post_cfg)
    post_device = lambda: model_nms_utils.post_processing(batch, cfg, len(names))
    post_ref = lambda: post_torch(post_cls, boxes, mapping, post_cfg)
    padded, ref = post_device(), post_ref()
    num = padded['num_pred'].tolist()
    same = all(n == len(r[1]) and torch.equal(padded['pred_boxes'][s, :n], r[0]) and torch.equal(padded['pred_labels'][s, :n], r[2])
               for s, (n, r) in enumerate(zip(num, ref)))
    result["post_above_threshold"] = [int((torch.sigmoid(x) >= post_cfg['SCORE_THRESH']).sum()) for x in post_cls]
    result["post_detections"], result["post_detections_equal"], result["post_box_columns"] = num, bool(same), int(boxes.shape[-1])
    result["post"] = timed_alternating({"device": post_device, "torch": post_ref}, args.steps, args.warmup)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
