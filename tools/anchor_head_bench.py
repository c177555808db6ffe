#!/usr/bin/env python
"""Times the anchor head at the KITTI shape of pointpillar.yaml -- a 248 x 216 map, three anchor classes of two rotations,
321 408 anchors a scene, B = 4, max_gt 48 -- on synthetic tensors.  One JSON line per (stage, variant): the median and the
minimum over --reps calls, wall clock between two device synchronisations, after --warmup calls; the two variants of a stage
alternate call by call, so that both see the same machine.

  targets   device: pda_anchor_assign_targets (two launches, two memsets).   torch: the reference-shaped composition on the
            same card: per scene the trailing-zero trim (a host read), per anchor class the anchors x gts IoU matrix, two
            argmaxes, the nonzero() compactions, the boolean-mask writes and the encoding of the positives.
  loss      device: pda_anchor_loss forward and backward.   torch: get_cls_layer_loss + get_box_reg_layer_loss as the
            reference composes them (one-hot scatter, focal loss, add_sin_difference, smooth L1, direction targets and
            cross-entropy) and autograd's backward, without the four .item() reads.
  decode    device: pda_anchor_decode.   torch: ResidualCoder.decode_torch against the repeated anchors and the direction
            classifier's bin.
--only STAGE runs one stage (for a `rocprofv3 --kernel-trace --stats` run of its own).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdanet_amd import anchor_head as ah, loss_utils  # noqa: E402
from pdanet_amd.box_coder_utils import ResidualCoder  # noqa: E402
from pdanet_amd.config import to_attr  # noqa: E402

PCR = [0, -39.68, -3, 69.12, 39.68, 1]
VS = [0.16, 0.16, 4]
NAMES = ['Car', 'Pedestrian', 'Cyclist']
SIZES = {'Car': [3.9, 1.6, 1.56], 'Pedestrian': [0.8, 0.6, 1.73], 'Cyclist': [1.76, 0.6, 1.73]}
BOTTOM = {'Car': -1.78, 'Pedestrian': -0.6, 'Cyclist': -0.6}
THRESH = {'Car': (0.6, 0.45), 'Pedestrian': (0.5, 0.35), 'Cyclist': (0.5, 0.35)}
HEAD = {
    'CLASS_AGNOSTIC': False, 'USE_DIRECTION_CLASSIFIER': True, 'DIR_OFFSET': 0.78539, 'DIR_LIMIT_OFFSET': 0.0, 'NUM_DIR_BINS': 2,
    'ANCHOR_GENERATOR_CONFIG': [
        {'class_name': n, 'anchor_sizes': [SIZES[n]], 'anchor_rotations': [0, 1.57], 'anchor_bottom_heights': [BOTTOM[n]],
         'align_center': False, 'feature_map_stride': 2, 'matched_threshold': THRESH[n][0], 'unmatched_threshold': THRESH[n][1]}
        for n in NAMES],
    'TARGET_ASSIGNER_CONFIG': {'NAME': 'AxisAlignedTargetAssigner', 'POS_FRACTION': -1.0, 'SAMPLE_SIZE': 512,
                               'NORM_BY_NUM_EXAMPLES': False, 'MATCH_HEIGHT': False, 'BOX_CODER': 'ResidualCoder'},
    'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0, 'dir_weight': 0.2, 'code_weights': [1.0] * 7}},
}


def synth(rng, B, m, n_live):
    gt = np.zeros((B, m, 8), np.float32)
    for b in range(B):
        k = n_live[b % len(n_live)]
        cls = rng.integers(0, 3, k)
        gt[b, :k, 0], gt[b, :k, 1] = rng.uniform(PCR[0] + 2, PCR[3] - 2, k), rng.uniform(PCR[1] + 2, PCR[4] - 2, k)
        gt[b, :k, 2] = rng.uniform(-1.2, -0.4, k)
        gt[b, :k, 3:6] = np.array([SIZES[NAMES[c]] for c in cls]) * rng.uniform(0.85, 1.15, (k, 3))
        gt[b, :k, 6], gt[b, :k, 7] = rng.uniform(-np.pi, np.pi, k), cls + 1
    return gt


def nearest_bev_iou(a, b):
    def aligned(x):
        r = (x[:, 6] - torch.floor(x[:, 6] / np.pi + 0.5) * np.pi).abs()
        dims = torch.where(r[:, None] < np.pi / 4, x[:, [3, 4]], x[:, [4, 3]])
        return torch.cat((x[:, 0:2] - dims / 2, x[:, 0:2] + dims / 2), dim=1)
    a, b = aligned(a), aligned(b)
    x_len = torch.clamp_min(torch.min(a[:, 2, None], b[None, :, 2]) - torch.max(a[:, 0, None], b[None, :, 0]), min=0)
    y_len = torch.clamp_min(torch.min(a[:, 3, None], b[None, :, 3]) - torch.max(a[:, 1, None], b[None, :, 1]), min=0)
    area_a, area_b = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    inter = x_len * y_len
    return inter / torch.clamp_min(area_a[:, None] + area_b[None, :] - inter, min=1e-6)


def targets_torch(anchors, gt_all, coder):
    """The reference's order of work: per scene, per anchor class."""
    out_t, out_l, out_w = [], [], []
    for k in range(gt_all.shape[0]):
        cur = gt_all[k]
        cnt = cur.shape[0] - 1
        while cnt > 0 and cur[cnt, :7].sum() == 0:              # the reference's trim: one host read per step
            cnt -= 1
        cur = cur[:cnt + 1]
        classes = cur[:, 7].int()
        per_class = []
        for c, anc in enumerate(anchors):
            fm = anc.shape[:3]
            anc = anc.view(-1, 7)
            mask = classes == c + 1
            gts, gcls = cur[mask, :7], classes[mask]
            n = anc.shape[0]
            labels = torch.full((n,), -1, dtype=torch.int32, device=anc.device)
            thr = THRESH[NAMES[c]]
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
                bg = (a2g_max < thr[1]).nonzero()[:, 0]
                labels[bg] = 0
                labels[forced] = gcls[force_gt]
            else:
                labels[:] = 0
            fg = (labels > 0).nonzero()[:, 0]
            targets = anc.new_zeros((n, 7))
            if gts.shape[0] > 0:
                targets[fg] = coder.encode_torch(gts[a2g[fg]], anc[fg])
            weights = anc.new_zeros((n,))
            weights[labels > 0] = 1.0
            per_class.append((labels.view(*fm, -1), targets.view(*fm, -1, 7), weights.view(*fm, -1)))
        out_l.append(torch.cat([p[0] for p in per_class], dim=-1).view(-1))
        out_t.append(torch.cat([p[1] for p in per_class], dim=-2).view(-1, 7))
        out_w.append(torch.cat([p[2] for p in per_class], dim=-1).view(-1))
    return torch.stack(out_l), torch.stack(out_t), torch.stack(out_w)


def loss_torch(cls_preds, box_preds, dir_preds, labels, targets, table, funcs):
    B, N = labels.shape
    cared, positives = labels >= 0, labels > 0
    cls_weights = ((labels == 0) * 1.0 + 1.0 * positives).float()
    norm = positives.sum(1, keepdim=True).float().clamp(min=1.0)
    cls_weights, reg_weights = cls_weights / norm, positives.float() / norm
    cls_targets = (labels * cared.type_as(labels)).long()
    one_hot = torch.zeros(B, N, 4, dtype=cls_preds.dtype, device=labels.device)
    one_hot.scatter_(-1, cls_targets.unsqueeze(-1), 1.0)
    cls_loss = funcs[0](cls_preds.view(B, N, 3), one_hot[..., 1:], weights=cls_weights).sum() / B
    anchors = table.view(1, -1, 7).repeat(B, 1, 1)
    bp = box_preds.view(B, N, 7)
    sin_p = torch.sin(bp[..., 6:7]) * torch.cos(targets[..., 6:7])
    sin_t = torch.cos(bp[..., 6:7]) * torch.sin(targets[..., 6:7])
    loc = funcs[1](torch.cat([bp[..., :6], sin_p], dim=-1), torch.cat([targets[..., :6], sin_t], dim=-1), weights=reg_weights)
    loc_loss = loc.sum() / B * 2.0
    rot_gt = targets[..., 6] + anchors[..., 6]
    val = rot_gt - HEAD['DIR_OFFSET']
    offset_rot = val - torch.floor(val / (2 * np.pi)) * (2 * np.pi)
    bins = torch.clamp(torch.floor(offset_rot / np.pi).long(), min=0, max=1)
    dir_targets = torch.zeros(B, N, 2, dtype=bp.dtype, device=bp.device)
    dir_targets.scatter_(-1, bins.unsqueeze(-1), 1.0)
    w = positives.type_as(bp)
    w = w / torch.clamp(w.sum(-1, keepdim=True), min=1.0)
    dir_loss = funcs[2](dir_preds.view(B, N, 2), dir_targets, weights=w).sum() / B * 0.2
    return cls_loss + loc_loss + dir_loss


def decode_torch(box_preds, dir_preds, table, coder):
    B = box_preds.shape[0]
    anchors = table.view(1, -1, 7).repeat(B, 1, 1)
    boxes = coder.decode_torch(box_preds.view(B, -1, 7), anchors)
    labels = torch.max(dir_preds.view(B, -1, 2), dim=-1)[1]
    period = 2 * np.pi / 2
    val = boxes[..., 6] - HEAD['DIR_OFFSET']
    rot = val - torch.floor(val / period + HEAD['DIR_LIMIT_OFFSET']) * period
    boxes[..., 6] = rot + HEAD['DIR_OFFSET'] + period * labels.to(boxes.dtype)
    return boxes


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--max-gt", type=int, default=48)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["targets", "loss", "decode"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("anchor_head_bench needs a GPU: there is no CPU path")
    B = a.batch
    pcr, vs = np.array(PCR, np.float64), np.array(VS, np.float64)
    grid = np.round((pcr[3:] - pcr[:3]) / vs).astype(np.int64)
    head = ah.AnchorHeadSingle(to_attr(HEAD), 64, 3, NAMES, grid, pcr, predict_boxes_when_training=False).cuda()
    rng = np.random.default_rng(0)
    gt = torch.from_numpy(synth(rng, B, a.max_gt, [a.max_gt, 20, 33, 8])).cuda()
    table = head.anchor_table(gt.device)
    N = table.shape[0]
    anchors_dev = [x.cuda() for x in head.anchors]
    cls_preds = torch.from_numpy((rng.standard_normal((B, N, 3)) - 4.6).astype(np.float32)).cuda()
    box_preds = torch.from_numpy((rng.standard_normal((B, N, 7)) * 0.2).astype(np.float32)).cuda()
    dir_preds = torch.from_numpy(rng.standard_normal((B, N, 2)).astype(np.float32)).cuda()
    targets = head.assign_targets(gt)
    coder = ResidualCoder()
    funcs = (loss_utils.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0),
             loss_utils.WeightedSmoothL1Loss(code_weights=[1.0] * 7).cuda(), loss_utils.WeightedCrossEntropyLoss())
    # the labels of both sides are compared before anything is timed (the count goes into every line)
    ref_l, _, _ = targets_torch(anchors_dev, gt, coder)
    mismatches = int((ref_l != targets['box_cls_labels']).sum())

    def loss_device():
        leaves = [t.detach().requires_grad_(True) for t in (cls_preds, box_preds, dir_preds)]
        head.forward_ret_dict = dict(targets, cls_preds=leaves[0], box_preds=leaves[1], dir_cls_preds=leaves[2])
        head.get_loss()[0].backward()

    def loss_ref():
        leaves = [t.detach().requires_grad_(True) for t in (cls_preds, box_preds, dir_preds)]
        loss_torch(*leaves, targets['box_cls_labels'], targets['box_reg_targets'], table, funcs).backward()

    stages = {
        'targets': (lambda: head.assign_targets(gt), lambda: targets_torch(anchors_dev, gt, coder)),
        'loss': (loss_device, loss_ref),
        'decode': (lambda: ah.anchor_decode(box_preds, dir_preds, table, HEAD['DIR_OFFSET'], HEAD['DIR_LIMIT_OFFSET']),
                   lambda: decode_torch(box_preds, dir_preds, table, coder)),
    }
    for stage, (dev_fn, ref_fn) in stages.items():
        if a.only and a.only != stage:
            continue
        for _ in range(a.warmup):
            dev_fn()
            ref_fn()
        ms = {'device': [], 'torch': []}
        for _ in range(a.reps):                              # alternating
            ms['device'].append(timed(dev_fn))
            ms['torch'].append(timed(ref_fn))
        for variant, v in ms.items():
            print(json.dumps({"bench": "anchor_head", "stage": stage, "variant": variant, "batch": B, "anchors": N,
                              "max_gt": a.max_gt, "positives": targets['num_pos'].tolist(), "label_mismatches": mismatches,
                              "ms_median": round(float(np.median(v)), 4), "ms_min": round(float(np.min(v)), 4), "reps": len(v),
                              "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
