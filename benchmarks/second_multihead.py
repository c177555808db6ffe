#!/usr/bin/env python
"""Times the dense head of kitti_models/second_multihead.yaml at the yaml's shape: 4 scenes, three one-class heads of
2 x 200 x 176 = 70 400 anchors each (211 200 a scene), SCORE_THRESH 0.1, NMS_PRE_MAXSIZE / NMS_POST_MAXSIZE 4096 / 500, on
synthetic tensors.

  train   targets + loss + backward.  device: pda_anchor_multi_assign_targets, pda_anchor_multi_loss and the gradient scaling
          (csrc/anchor_head.hip).  torch: the reference's order of work on the same card -- per scene the trailing-zero trim (host
          reads), per anchor class the anchors x gts IoU matrix, two argmaxes, nonzero() compactions, boolean-mask writes and the
          encoding; then per head the one-hot slice, focal loss, add_sin_difference, smooth L1, direction targets and
          cross-entropy, and autograd's backward (without the reference's .item() reads).
  post    post-processing with MULTI_CLASSES_NMS.  device: model_nms_utils.post_processing (one sort per head, one pda_nms_bev
          over all (scene, head, class) problems, pda_multi_nms_compact), no host read.  torch: the reference's loop over
          scenes, heads and classes -- mask, topk, nms_gpu (this repository's, with its host read of the count, where the
          reference copies the mask to the host), index back, concatenate.

The sides alternate inside one process; every figure is a wall-clock time between two device synchronisations per call (the
composed side reads the host, so device events alone would not see its waits), `--steps` calls after `--warmup` calls, in
milliseconds: median, minimum, maximum.  The labels of the two target assignments and the detections of the two post-processings
are compared before anything is timed.  A measurement, not a gate: prints one JSON line.

    python benchmarks/second_multihead.py [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from pdanet_amd import anchor_head_multi as ahm, iou3d_nms_utils, loss_utils, model_nms_utils      # noqa: E402
from pdanet_amd.box_coder_utils import ResidualCoder                                                   # noqa: E402
from pdanet_amd.config import to_attr                                                                  # noqa: E402
# the synthetic gt boxes (inside this range too), the classes' sizes and thresholds, and the torch IoU of the anchor head's tool
from anchor_head_bench import NAMES, SIZES, THRESH, nearest_bev_iou, synth                             # noqa: E402

PCR, VOXEL = [0, -40, -3, 70.4, 40, 1], [0.05, 0.05, 0.1]
HEAD = {
    'CLASS_AGNOSTIC': False, 'USE_DIRECTION_CLASSIFIER': True, 'DIR_OFFSET': 0.78539, 'DIR_LIMIT_OFFSET': 0.0, 'NUM_DIR_BINS': 2,
    'USE_MULTIHEAD': True, 'SEPARATE_MULTIHEAD': True, 'SHARED_CONV_NUM_FILTER': 64,
    'ANCHOR_GENERATOR_CONFIG': [
        {'class_name': n, 'anchor_sizes': [SIZES[n]], 'anchor_rotations': [0, 1.57], 'anchor_bottom_heights': [-1.6],
         'align_center': False, 'feature_map_stride': 8, 'matched_threshold': THRESH[n][0], 'unmatched_threshold': THRESH[n][1]}
        for n in NAMES],
    'RPN_HEAD_CFGS': [{'HEAD_CLS_NAME': [n]} for n in NAMES],
    'TARGET_ASSIGNER_CONFIG': {'NAME': 'AxisAlignedTargetAssigner', 'POS_FRACTION': -1.0, 'SAMPLE_SIZE': 512,
                               'NORM_BY_NUM_EXAMPLES': False, 'MATCH_HEIGHT': False, 'BOX_CODER': 'ResidualCoder'},
    'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0, 'dir_weight': 0.2, 'code_weights': [1.0] * 7}},
}
POST = {'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'SCORE_THRESH': 0.1, 'OUTPUT_RAW_SCORE': False,
        'NMS_CONFIG': {'MULTI_CLASSES_NMS': True, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.1, 'NMS_PRE_MAXSIZE': 4096,
                       'NMS_POST_MAXSIZE': 500}}


def targets_torch(class_tables, gt_all, coder):
    """The reference's order of work with use_multihead: per scene, per anchor class over its class-major rows."""
    out_l, out_t = [], []
    for k in range(gt_all.shape[0]):
        cur = gt_all[k]
        cnt = cur.shape[0] - 1
        while cnt > 0 and cur[cnt, :7].sum() == 0:              # the reference's trim: one host read per step
            cnt -= 1
        cur = cur[:cnt + 1]
        classes = cur[:, 7].int()
        labels_k, targets_k = [], []
        for c, anc in enumerate(class_tables):
            mask = classes == c + 1
            gts, gcls = cur[mask, :7], classes[mask]
            n = anc.shape[0]
            labels = torch.full((n,), -1, dtype=torch.int32, device=anc.device)
            thr = THRESH[NAMES[c]]
            targets = anc.new_zeros((n, 7))
            if gts.shape[0] > 0:
                iou = nearest_bev_iou(anc, gts)
                a2g = iou.argmax(dim=1)
                a2g_max = iou[torch.arange(n, device=anc.device), a2g]
                g2a = iou.argmax(dim=0)
                g2a_max = iou[g2a, torch.arange(gts.shape[0], device=anc.device)]
                g2a_max[g2a_max == 0] = -1
                forced = (iou == g2a_max).nonzero()[:, 0]
                force_gt = a2g[forced]
                labels[forced] = gcls[force_gt]
                pos = a2g_max >= thr[0]
                labels[pos] = gcls[a2g[pos]]
                labels[(a2g_max < thr[1]).nonzero()[:, 0]] = 0
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


def loss_torch(cls_preds, box_preds, dir_preds, labels, targets, table, funcs):
    """get_cls_layer_loss + get_box_reg_layer_loss of anchor_head_multi.py for a separate multihead of one-class heads."""
    B, N = labels.shape
    cared, positives = labels >= 0, labels > 0
    norm = positives.sum(1, keepdim=True).float().clamp(min=1.0)
    cls_weights, reg_weights = cared.float() / norm, positives.float() / norm
    one_hot = torch.zeros(B, N, 4, dtype=cls_preds[0].dtype, device=labels.device)
    one_hot.scatter_(-1, (labels * cared.type_as(labels)).long().unsqueeze(-1), 1.0)
    one_hot = one_hot[..., 1:]
    rot_gt = targets[..., 6] + table.view(1, -1, 7)[..., 6]
    val = rot_gt - HEAD['DIR_OFFSET']
    offset_rot = val - torch.floor(val / (2 * np.pi)) * (2 * np.pi)
    bins = torch.clamp(torch.floor(offset_rot / np.pi).long(), min=0, max=1)
    dir_targets = torch.zeros(B, N, 2, dtype=targets.dtype, device=targets.device)
    dir_targets.scatter_(-1, bins.unsqueeze(-1), 1.0)
    start, total = 0, 0
    for h, (cp, bp, dp) in enumerate(zip(cls_preds, box_preds, dir_preds)):
        n = cp.shape[1]
        rows = slice(start, start + n)
        total = total + funcs[0](cp, one_hot[:, rows, h:h + 1], weights=cls_weights[:, rows]).sum() / B
        tg = targets[:, rows]
        sin_p = torch.sin(bp[..., 6:7]) * torch.cos(tg[..., 6:7])
        sin_t = torch.cos(bp[..., 6:7]) * torch.sin(tg[..., 6:7])
        loc = funcs[1](torch.cat([bp[..., :6], sin_p], dim=-1), torch.cat([tg[..., :6], sin_t], dim=-1), weights=reg_weights[:, rows])
        total = total + loc.sum() / B * 2.0
        total = total + funcs[2](dp, dir_targets[:, rows], weights=reg_weights[:, rows]).sum() / B * 0.2
        start += n
    return total


def post_torch(cls_preds, box_preds, mapping, cfg):
    """detector3d_template.post_processing with MULTI_CLASSES_NMS over model_nms_utils.multi_classes_nms: scenes, heads, classes."""
    nms = cfg['NMS_CONFIG']
    result = []
    for s in range(box_preds.shape[0]):
        scores, labels, boxes = [], [], []
        start = 0
        for x, m in zip(cls_preds, mapping):
            cur = torch.sigmoid(x[s])
            cur_boxes = box_preds[s, start:start + cur.shape[0]]
            for k in range(cur.shape[1]):
                mask = cur[:, k] >= cfg['SCORE_THRESH']
                box_scores, masked_boxes = cur[mask, k], cur_boxes[mask]
                if box_scores.shape[0] > 0:
                    top, idx = torch.topk(box_scores, k=min(nms['NMS_PRE_MAXSIZE'], box_scores.shape[0]))
                    keep, _ = iou3d_nms_utils.nms_gpu(masked_boxes[idx][:, 0:7], top, nms['NMS_THRESH'])
                    sel = idx[keep[:nms['NMS_POST_MAXSIZE']]]
                    scores.append(box_scores[sel])
                    labels.append(m[k].expand(len(sel)))
                    boxes.append(masked_boxes[sel])
            start += cur.shape[0]
        result.append((torch.cat(boxes), torch.cat(scores), torch.cat(labels)))
    return result


def timed_alternating(fns, steps, warmup):
    """name -> [median, min, max] wall-clock ms per call between two device synchronisations; the sides take turns."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)] for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--max-gt", type=int, default=48)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/second_multihead.py needs the GPU: a CPU run gives no time")
    torch.cuda.set_device(0)
    B = args.batch
    pcr, vs = np.array(PCR, np.float64), np.array(VOXEL, np.float64)
    grid = np.round((pcr[3:] - pcr[:3]) / vs).astype(np.int64)
    head = ahm.AnchorHeadMulti(to_attr(HEAD), 512, 3, NAMES, grid, pcr, predict_boxes_when_training=False).cuda()
    rng = np.random.default_rng(0)
    gt = torch.from_numpy(synth(rng, B, args.max_gt, [args.max_gt, 20, 33, 8])).cuda()
    table = head.anchor_table(gt.device)
    rows = head.head_rows
    first = np.concatenate([[0], np.cumsum(rows)])
    class_tables = [table[first[c]:first[c + 1]] for c in range(3)]
    dev = lambda x: torch.from_numpy(x.astype(np.float32)).cuda()
    cls_preds = [dev(rng.standard_normal((B, n, 1)) - 4.6) for n in rows]
    box_preds = [dev(rng.standard_normal((B, n, 7)) * 0.2) for n in rows]
    dir_preds = [dev(rng.standard_normal((B, n, 2))) for n in rows]
    coder = ResidualCoder()
    funcs = (loss_utils.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0),
             loss_utils.WeightedSmoothL1Loss(code_weights=[1.0] * 7).cuda(), loss_utils.WeightedCrossEntropyLoss())
    targets = head.assign_targets(gt)
    ref_labels, ref_targets = targets_torch(class_tables, gt, coder)
    result = {"benchmark": "second_multihead", "batch": B, "anchors": int(table.shape[0]), "heads": rows, "max_gt": args.max_gt,
              "steps": args.steps, "warmup": args.warmup, "unit": "wall-clock ms per call (median, min, max)",
              "device": torch.cuda.get_device_name(0), "positives": targets['num_pos'].tolist(),
              "label_mismatches": int((ref_labels != targets['box_cls_labels']).sum())}

    def leaves():
        return [[t.detach().requires_grad_(True) for t in parts] for parts in (cls_preds, box_preds, dir_preds)]

    def train_device():
        c, b, d = leaves()
        head.forward_ret_dict = dict(head.assign_targets(gt), cls_preds=c, box_preds=b, dir_cls_preds=d)
        loss = head.get_loss()[0]
        loss.backward()
        return loss

    def train_torch():
        c, b, d = leaves()
        labels, tg = targets_torch(class_tables, gt, coder)
        loss = loss_torch(c, b, d, labels, tg, table, funcs)
        loss.backward()
        return loss

    result["loss_device_torch"] = [float(train_device().detach()), float(train_torch().detach())]
    result["train"] = timed_alternating({"device": train_device, "torch": train_torch}, args.steps, args.warmup)

    # post-processing: logits around the head's initial bias with a tail above the threshold, decoded boxes of small codes
    post_cls = [dev(rng.standard_normal((B, n, 1)) * 1.6 - 4.6) for n in rows]
    with torch.no_grad():
        _, boxes = head.generate_predicted_boxes(B, post_cls, box_preds, dir_preds)
    mapping = [h.head_label_indices for h in head.rpn_heads]
    batch = {'batch_size': B, 'batch_cls_preds': post_cls, 'batch_box_preds': boxes, 'cls_preds_normalized': False,
             'multihead_label_mapping': mapping}
    cfg = to_attr(POST)
    post_device = lambda: model_nms_utils.post_processing(batch, cfg, 3)
    post_ref = lambda: post_torch(post_cls, boxes, mapping, POST)
    padded, ref = post_device(), post_ref()
    num = padded['num_pred'].tolist()
    same = all(n == len(r[1]) and torch.equal(padded['pred_boxes'][s, :n], r[0]) and torch.equal(padded['pred_labels'][s, :n], r[2])
               for s, (n, r) in enumerate(zip(num, ref)))
    result["post_above_threshold"] = [int((torch.sigmoid(x) >= POST['SCORE_THRESH']).sum()) for x in post_cls]
    result["post_detections"], result["post_detections_equal"] = num, bool(same)
    result["post"] = timed_alternating({"device": post_device, "torch": post_ref}, args.steps, args.warmup)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
