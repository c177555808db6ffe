#!/usr/bin/env python
"""Times the CenterPoint pillar tail at the Waymo shape of centerpoint_dyn_pillar_1x.yaml -- a 468 x 468 map, stride 1, one head
of three classes, B = 2, 500 objects a scene, 64 pillar channels -- on synthetic tensors.  One JSON line per (stage,
variant): the median and the minimum over --reps calls, wall clock between two device synchronisations, after --warmup
calls; the two variants of a stage alternate call by call, so that both see the same machine.

  scatter   device: pda_pillar_scatter_fwd (+ the fill).   torch: the reference-shaped per-scene loop (mask, index, transposed
            assignment, stack) on the same tensors, with batch_size known (no .item()).
  targets   device: pda_center_assign_targets (+ the fill).   host: the reference-shaped loop: boxes to the host, a Python
            loop over scenes and objects, each Gaussian drawn with numpy, four uploads per scene.
  loss      device: focal_loss + reg_loss forward and backward.   torch: clamp(sigmoid), neg_loss_cornernet, cat, the
            channel-last copy and gather of _transpose_and_gather_feat, _reg_loss, and autograd's backward.
  decode    device: generate_predicted_boxes (topk on the logits, pda_center_decode, batched NMS).   torch: sigmoid, the
            two-stage _topk, five channel-last copies and gathers, the masks, then per scene boolean indexing and nms_gpu.
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
from pdanet_amd import iou3d_nms_utils as iu  # noqa: E402
from pdanet_amd.center_head import CenterHead  # noqa: E402
from pdanet_amd.config import to_attr  # noqa: E402
from pdanet_amd.pointpillar_scatter import pillar_scatter  # noqa: E402

PCR = [-74.88, -74.88, -2.0, 74.88, 74.88, 4.0]
VS = [0.32, 0.32, 6.0]
NAMES = ['Vehicle', 'Pedestrian', 'Cyclist']
DIMS = np.array([(4.7, 2.1, 1.7), (0.9, 0.85, 1.75), (1.8, 0.85, 1.75)])
HEAD = {
    'CLASS_AGNOSTIC': False, 'CLASS_NAMES_EACH_HEAD': [NAMES], 'SHARED_CONV_CHANNEL': 64, 'USE_BIAS_BEFORE_NORM': True,
    'NUM_HM_CONV': 2,
    'SEPARATE_HEAD_CFG': {'HEAD_ORDER': ['center', 'center_z', 'dim', 'rot'],
                          'HEAD_DICT': {'center': {'out_channels': 2, 'num_conv': 2}, 'center_z': {'out_channels': 1, 'num_conv': 2},
                                        'dim': {'out_channels': 3, 'num_conv': 2}, 'rot': {'out_channels': 2, 'num_conv': 2}}},
    'TARGET_ASSIGNER_CONFIG': {'FEATURE_MAP_STRIDE': 1, 'NUM_MAX_OBJS': 500, 'GAUSSIAN_OVERLAP': 0.1, 'MIN_RADIUS': 2},
    'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0, 'code_weights': [1.0] * 8}},
    'POST_PROCESSING': {'SCORE_THRESH': 0.1, 'POST_CENTER_LIMIT_RANGE': [-80, -80, -10.0, 80, 80, 10.0], 'MAX_OBJ_PER_SAMPLE': 500,
                        'NMS_CONFIG': {'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.7, 'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 500}},
}


def synth(rng, B, n_obj, H, W, C, n_pillars):
    gt = np.zeros((B, n_obj, 8), np.float32)
    cls = rng.integers(0, 3, (B, n_obj))
    gt[..., 0], gt[..., 1] = rng.uniform(PCR[0], PCR[3], (B, n_obj)), rng.uniform(PCR[1], PCR[4], (B, n_obj))
    gt[..., 2] = rng.uniform(-1, 1, (B, n_obj))
    gt[..., 3:6] = DIMS[cls] * rng.uniform(0.8, 1.2, (B, n_obj, 3))
    gt[..., 6], gt[..., 7] = rng.uniform(-np.pi, np.pi, (B, n_obj)), cls + 1
    preds = {'hm': (rng.standard_normal((B, 3, H, W)) * 1.5 - 4.5).astype(np.float32)}
    for k, c in (('center', 2), ('center_z', 1), ('dim', 3), ('rot', 2)):
        preds[k] = (rng.standard_normal((B, c, H, W)) * 0.5).astype(np.float32)
    cells = np.sort(np.concatenate([b * H * W + rng.permutation(H * W)[:n_pillars] for b in range(B)]))
    coords = np.zeros((len(cells), 4), np.int32)
    coords[:, 0], coords[:, 2], coords[:, 3] = cells // (H * W), (cells % (H * W)) // W, cells % W
    feats = rng.standard_normal((len(cells), C)).astype(np.float32)
    return gt, preds, feats, coords


def scatter_torch(feats, coords, B, C, ny, nx):
    out = []
    for b in range(B):
        plane = torch.zeros(C, ny * nx, dtype=feats.dtype, device=feats.device)
        m = coords[:, 0] == b
        c = coords[m]
        plane[:, (c[:, 1] + c[:, 2] * nx + c[:, 3]).long()] = feats[m].t()
        out.append(plane)
    return torch.stack(out, 0).view(B, C, ny, nx)


def gaussian_radius(h, w, o):
    b1, c1 = h + w, w * h * (1 - o) / (1 + o)
    r1 = (b1 + (b1 ** 2 - 4 * c1).sqrt()) / 2
    b2, c2 = 2 * (h + w), (1 - o) * w * h
    r2 = (b2 + (b2 ** 2 - 16 * c2).sqrt()) / 2
    a3, b3, c3 = 4 * o, -2 * o * (h + w), (o - 1) * w * h
    r3 = (b3 + (b3 ** 2 - 4 * a3 * c3).sqrt()) / 2
    return torch.min(torch.min(r1, r2), r3)


def targets_host(gt, H, W, K=500, o=0.1, min_radius=2):
    """The reference's order of work for one head of all classes: per scene on the host, per object a numpy Gaussian."""
    outs = [[], [], [], []]
    for b in range(gt.shape[0]):
        g = gt[b].cpu()
        g = g[g[:, -1] > 0]
        hm, ret = g.new_zeros(3, H, W), g.new_zeros(K, 8)
        inds, mask = g.new_zeros(K).long(), g.new_zeros(K).long()
        cx = ((g[:, 0] - PCR[0]) / VS[0] / 1).clamp(min=0, max=W - 0.5)
        cy = ((g[:, 1] - PCR[1]) / VS[1] / 1).clamp(min=0, max=H - 0.5)
        ctr = torch.stack([cx, cy], -1)
        ci = ctr.int()
        dx, dy = g[:, 3] / VS[0], g[:, 4] / VS[1]
        radius = gaussian_radius(dx, dy, o).int().clamp_min(min_radius)
        for k in range(min(K, g.shape[0])):
            if dx[k] <= 0 or dy[k] <= 0:
                continue
            r = radius[k].item()
            x, y = int(ctr[k, 0]), int(ctr[k, 1])
            yy, xx = np.ogrid[-r:r + 1, -r:r + 1]
            gauss = np.exp(-(xx * xx + yy * yy) / (2 * ((2 * r + 1) / 6) ** 2))
            left, right, top, bottom = min(x, r), min(W - x, r + 1), min(y, r), min(H - y, r + 1)
            plane = hm[(g[k, -1] - 1).long()][y - top:y + bottom, x - left:x + right]
            torch.max(plane, torch.from_numpy(gauss[r - top:r + bottom, r - left:r + right]).float(), out=plane)
            inds[k], mask[k] = ci[k, 1] * W + ci[k, 0], 1
            ret[k, 0:2] = ctr[k] - ci[k].float()
            ret[k, 2], ret[k, 3:6] = g[k, 2], g[k, 3:6].log()
            ret[k, 6], ret[k, 7] = torch.cos(g[k, 6]), torch.sin(g[k, 6])
        for lst, t in zip(outs, (hm, ret, inds, mask)):
            lst.append(t.to(gt.device))
    return [torch.stack(x, 0) for x in outs]


def gather_feat(feat, ind):
    feat = feat.permute(0, 2, 3, 1).contiguous()
    feat = feat.view(feat.size(0), -1, feat.size(3))
    return feat.gather(1, ind.unsqueeze(2).expand(ind.size(0), ind.size(1), feat.size(2)))


def loss_torch(preds, hm_t, tb, inds, masks):
    pred = torch.clamp(preds['hm'].sigmoid(), min=1e-4, max=1 - 1e-4)
    pos, neg = hm_t.eq(1).float(), hm_t.lt(1).float()
    pos_loss = (torch.log(pred) * torch.pow(1 - pred, 2) * pos).sum()
    neg_loss = (torch.log(1 - pred) * torch.pow(pred, 2) * torch.pow(1 - hm_t, 4) * neg).sum()
    num_pos = pos.sum()
    hm_loss = torch.where(num_pos == 0, -neg_loss, -(pos_loss + neg_loss) / num_pos.clamp(min=1))     # the branch without its read
    boxes = torch.cat([preds[k] for k in HEAD['SEPARATE_HEAD_CFG']['HEAD_ORDER']], dim=1)
    regr = gather_feat(boxes, inds)
    num = masks.float().sum()
    m = masks.unsqueeze(2).expand_as(tb).float() * (~torch.isnan(tb)).float()
    loss = torch.abs(regr * m - tb * m).transpose(2, 0).sum(dim=2).sum(dim=1) / torch.clamp_min(num, min=1.0)
    return hm_loss + (loss * loss.new_tensor([1.0] * 8)).sum() * 2.0


def decode_torch(preds, K, nms_cfg, limit, thresh):
    hm = preds['hm'].sigmoid()
    B, C, H, W = hm.shape
    s1, i1 = torch.topk(hm.flatten(2, 3), K)
    i1 = i1 % (H * W)
    ys, xs = (i1 // W).float(), (i1 % W).int().float()
    score, i2 = torch.topk(s1.view(B, -1), K)
    cls = (i2 // K).int()
    inds, ys, xs = (t.view(B, -1).gather(1, i2) for t in (i1, ys, xs))
    center, rot, z, dim = (gather_feat(preds[k] if k != 'dim' else preds[k].exp(), inds) for k in ('center', 'rot', 'center_z', 'dim'))
    angle = torch.atan2(rot[..., 1:2], rot[..., 0:1])
    x = (xs.view(B, K, 1) + center[..., 0:1]) * 1 * VS[0] + PCR[0]
    y = (ys.view(B, K, 1) + center[..., 1:2]) * 1 * VS[1] + PCR[1]
    boxes = torch.cat([x, y, z, dim, angle], dim=-1)
    mask = (boxes[..., :3] >= limit[:3]).all(2) & (boxes[..., :3] <= limit[3:]).all(2) & (score > thresh)
    out = []
    for b in range(B):
        bb, ss, ll = boxes[b, mask[b]], score[b, mask[b]], cls[b, mask[b]]
        if ss.shape[0]:
            top, idx = torch.topk(ss, k=min(nms_cfg['NMS_PRE_MAXSIZE'], ss.shape[0]))
            keep, _ = iu.nms_gpu(bb[idx][:, 0:7], top, nms_cfg['NMS_THRESH'])
            sel = idx[keep[:nms_cfg['NMS_POST_MAXSIZE']]]
            bb, ss, ll = bb[sel], ss[sel], ll[sel]
        out.append((bb, ss, ll + 1))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--map", type=int, default=468)
    ap.add_argument("--objects", type=int, default=500)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--pillars", type=int, default=30000, help="pillars a scene")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3, help="calls of the host loop of target assignment")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["scatter", "targets", "loss", "decode"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("center_head_bench needs a GPU: there is no CPU path")
    B, H, W = a.batch, a.map, a.map
    gt, preds, feats, coords = synth(np.random.default_rng(0), B, a.objects, H, W, a.channels, a.pillars)
    gt, feats, coords = torch.from_numpy(gt).cuda(), torch.from_numpy(feats).cuda(), torch.from_numpy(coords).cuda()
    preds = {k: torch.from_numpy(v).cuda() for k, v in preds.items()}
    head = CenterHead(to_attr(HEAD), 16, 3, NAMES, [W, H, 1], PCR, VS, predict_boxes_when_training=False).cuda()
    targets = head.assign_targets(gt, feature_map_size=(H, W))
    hm_t, tb, inds, masks = (targets[k][0] for k in ('heatmaps', 'target_boxes', 'inds', 'masks'))
    limit = torch.tensor(HEAD['POST_PROCESSING']['POST_CENTER_LIMIT_RANGE'], dtype=torch.float32, device='cuda')
    pp = HEAD['POST_PROCESSING']

    def loss_device():
        leaves = {k: v.detach().requires_grad_(True) for k, v in preds.items()}
        head.forward_ret_dict = {'pred_dicts': [leaves], 'target_dicts': targets}
        head.get_loss()[0].backward()

    def loss_ref():
        leaves = {k: v.detach().requires_grad_(True) for k, v in preds.items()}
        loss_torch(leaves, hm_t, tb, inds, masks).backward()

    stages = {
        'scatter': (lambda: pillar_scatter(feats, coords, B, H, W), lambda: scatter_torch(feats, coords, B, a.channels, H, W), 'torch'),
        'targets': (lambda: head.assign_targets(gt, feature_map_size=(H, W)), lambda: targets_host(gt, H, W), 'host'),
        'loss': (loss_device, loss_ref, 'torch'),
        'decode': (lambda: head.generate_predicted_boxes(B, [preds]),
                   lambda: decode_torch(preds, pp['MAX_OBJ_PER_SAMPLE'], pp['NMS_CONFIG'], limit, pp['SCORE_THRESH']), 'torch'),
    }
    for stage, (dev_fn, ref_fn, ref_name) in stages.items():
        if a.only and a.only != stage:
            continue
        reps = a.host_reps if stage == 'targets' else a.reps
        for _ in range(a.warmup):
            dev_fn()
        for _ in range(1 if stage == 'targets' else a.warmup):
            ref_fn()
        ms = {'device': [], ref_name: []}
        for i in range(max(reps, a.reps)):                   # alternating
            ms['device'].append(timed(dev_fn))
            if i < reps:
                ms[ref_name].append(timed(ref_fn))
        for variant, v in ms.items():
            print(json.dumps({"bench": "center_head", "stage": stage, "variant": variant, "batch": B, "map": [H, W],
                              "objects": a.objects, "pillars": int(feats.shape[0]), "ms_median": round(float(np.median(v)), 4),
                              "ms_min": round(float(np.min(v)), 4), "reps": len(v), "warmup": a.warmup,
                              "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
