"""ProposalTargetLayer (pcdet/models/roi_heads/target_assigner/proposal_target_layer.py) for the whole batch on the device:
the max IoU of every RoI against its scene's ground truth (per class with SAMPLE_ROI_BY_EACH_CLASS), the fg / hard-bg /
easy-bg sampling down to ROI_PER_IMAGE, the gathers, the labels, and the canonical transformation that
RoIHeadTemplate.assign_targets (roi_head_template.py:104-134) applies afterwards -- two launches (csrc/roi_targets.hip)
and no host read, where the reference loops over scenes and classes in Python with .item(), nonzero() and per-scene uploads
of host draws.

Draws, the convention of the data stages (data_processor.py): with `draws` the caller passes the reference's own draws and
the sampled indices are the reference's (explicit mode); otherwise they are generated on the device from a 64-bit `seed`,
drawn from torch's CPU generator when not given, so torch.manual_seed makes a run reproducible.  Seeded mode follows the
reference's branch rules and distributions (a uniform sample without replacement of the fg list, uniform draws with
replacement elsewhere), not numpy's or torch's bit streams.

Kept as the reference has them: the three masks are literal, so with CLS_FG_THRESH < REG_FG_THRESH a RoI can be picked as
foreground and as hard background; zero-padded RoI rows are ordinary RoIs with IoU 0; a RoI whose class has no GT in the
scene gets IoU 0 and GT row 0."""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from .pointnet2_batch_cuda import F32, I32, _call, _chk

I64 = torch.int64
MAX_ROIS = 4096                       # csrc/roi_targets.hip ROI_MAX_M
_SCORE_TYPES = {'cls': 0, 'roi_iou': 1}
DRAW_KEYS = ('perm', 'fg_rand', 'hard_draw', 'easy_draw')


def _boxes(rois, gt_boxes):
    if not isinstance(rois, torch.Tensor) or rois.dim() != 3 or not isinstance(gt_boxes, torch.Tensor) or gt_boxes.dim() != 3:
        raise TypeError("rois must be (B, M, 7) and gt_boxes (B, T, 8) tensors")
    if rois.shape[-1] > 7 or gt_boxes.shape[-1] > 8:
        raise NotImplementedError("boxes with velocities are not supported")
    if rois.shape[-1] != 7 or gt_boxes.shape[-1] != 8:
        raise ValueError("rois must be (B, M, 7) and gt_boxes (B, T, 8), got %s and %s" % (tuple(rois.shape), tuple(gt_boxes.shape)))
    if rois.shape[0] != gt_boxes.shape[0]:
        raise ValueError("rois and gt_boxes disagree on the batch size")
    if rois.shape[1] > MAX_ROIS:
        raise ValueError("at most %d RoIs a scene, got %d" % (MAX_ROIS, rois.shape[1]))
    return rois.contiguous(), gt_boxes.contiguous()


def roi_max_iou(rois, roi_labels, gt_boxes, by_class=True):
    """rois (B, M, 7) float32, roi_labels (B, M) int64, gt_boxes (B, T, 8) float32 with the class in the last column ->
    max_overlaps (B, M) float32, gt_assignment (B, M) int32: per scene get_max_iou_with_same_class (by_class) or
    boxes_iou3d_gpu(...).max(1) against the GT trimmed as the reference trims it.  One launch, no host read."""
    rois, gt = _boxes(rois, gt_boxes)
    B, M, T = rois.shape[0], rois.shape[1], gt.shape[1]
    labels = roi_labels.reshape(B, M).contiguous()
    max_overlaps = torch.empty((B, M), dtype=F32, device=rois.device)
    gt_assignment = torch.empty((B, M), dtype=I32, device=rois.device)
    _call("pda_roi_max_iou", rois, _chk(rois, "rois", F32), _chk(labels, "roi_labels", I64), _chk(gt, "gt_boxes", F32), 8,
          int(bool(by_class)), _chk(max_overlaps, "max_overlaps", F32), _chk(gt_assignment, "gt_assignment", I32), B, M, T)
    return max_overlaps, gt_assignment


def _pad_draws(draws, B, M, R, device):
    """draws: dict of DRAW_KEYS, each one host array per scene (a (B, n) array or a list; a missing key counts as empty)
    -> the four padded device tensors the kernel reads."""
    shapes = {'perm': (M, np.int32), 'fg_rand': (R, np.float64), 'hard_draw': (R, np.int64), 'easy_draw': (R, np.int64)}
    out = []
    for key in DRAW_KEYS:
        width, dtype = shapes[key]
        v = draws.get(key)
        host = np.zeros((B, width), dtype)
        if v is not None:
            if len(v) != B:
                raise ValueError("draws[%r] needs one entry per scene" % key)
            for s in range(B):
                row = np.asarray(v[s]).reshape(-1)
                if row.shape[0] > width:
                    raise ValueError("draws[%r][%d] has %d entries, at most %d" % (key, s, row.shape[0], width))
                host[s, :row.shape[0]] = row
        out.append(torch.from_numpy(host).to(device))
    return out


def roi_sample_targets(rois, roi_scores, roi_labels, gt_boxes, max_overlaps, gt_assignment, cfg, seed=None, draws=None):
    """subsample_rois and everything after it for every scene (see the module docstring).  cfg: the TARGET_CONFIG keys
    ROI_PER_IMAGE, FG_RATIO, HARD_BG_RATIO, REG_FG_THRESH, CLS_FG_THRESH, CLS_BG_THRESH, CLS_BG_THRESH_LO, CLS_SCORE_TYPE.
    Returns the targets dict with 'sampled_inds' (B, R) int32 and 'status' (B) int32 added.  One launch, no host read."""
    rois, gt = _boxes(rois, gt_boxes)
    B, M, T = rois.shape[0], rois.shape[1], gt.shape[1]
    R = int(cfg['ROI_PER_IMAGE'])
    if R <= 0:
        raise ValueError("ROI_PER_IMAGE must be positive, got %d" % R)
    score_type = _SCORE_TYPES[cfg['CLS_SCORE_TYPE']]
    dev = rois.device
    scores = roi_scores.reshape(B, M).contiguous()
    labels = roi_labels.reshape(B, M).contiguous()
    out = {
        'rois': torch.empty((B, R, 7), dtype=F32, device=dev),
        'gt_of_rois': torch.empty((B, R, 8), dtype=F32, device=dev),
        'gt_iou_of_rois': torch.empty((B, R), dtype=F32, device=dev),
        'roi_scores': torch.empty((B, R), dtype=F32, device=dev),
        'roi_labels': torch.empty((B, R), dtype=I64, device=dev),
        'reg_valid_mask': torch.empty((B, R), dtype=I64, device=dev),
        'rcnn_cls_labels': torch.empty((B, R), dtype=I64 if score_type == 0 else F32, device=dev),
        'gt_of_rois_src': torch.empty((B, R, 8), dtype=F32, device=dev),
        'sampled_inds': torch.empty((B, R), dtype=I32, device=dev),
        'status': torch.zeros((B,), dtype=I32, device=dev),
    }
    if B == 0 or M == 0:
        for v in out.values():
            v.zero_()
        return out
    if draws is not None:
        perm, fg_rand, hard, easy = _pad_draws(draws, B, M, R, dev)
        ptrs = [_chk(perm, "perm", I32), _chk(fg_rand, "fg_rand", torch.float64), _chk(hard, "hard_draw", I64),
                _chk(easy, "easy_draw", I64)]
        seed = 0
    else:
        ptrs = [None] * 4
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())   # CPU generator: no device read
    fg_per_image = int(np.round(cfg['FG_RATIO'] * R))
    _call("pda_roi_sample_targets", rois, _chk(rois, "rois", F32), _chk(scores, "roi_scores", F32), _chk(labels, "roi_labels", I64),
          _chk(gt, "gt_boxes", F32), 8, _chk(max_overlaps, "max_overlaps", F32), _chk(gt_assignment, "gt_assignment", I32),
          R, fg_per_image, float(cfg['HARD_BG_RATIO']), float(cfg['REG_FG_THRESH']), float(cfg['CLS_FG_THRESH']),
          float(cfg['CLS_BG_THRESH']), float(cfg['CLS_BG_THRESH_LO']), score_type, *ptrs,
          ctypes.c_uint64(int(seed) & (2 ** 64 - 1)),
          _chk(out['rois'], "rois", F32), _chk(out['gt_of_rois_src'], "gt_of_rois_src", F32),
          _chk(out['gt_of_rois'], "gt_of_rois", F32), _chk(out['gt_iou_of_rois'], "gt_iou_of_rois", F32),
          _chk(out['roi_scores'], "roi_scores", F32), _chk(out['roi_labels'], "roi_labels", I64),
          _chk(out['reg_valid_mask'], "reg_valid_mask", I64), out['rcnn_cls_labels'].data_ptr(),
          _chk(out['sampled_inds'], "sampled_inds", I32), _chk(out['status'], "status", I32), B, M, T)
    return out


class ProposalTargetLayer(nn.Module):
    def __init__(self, roi_sampler_cfg):
        super().__init__()
        self.roi_sampler_cfg = roi_sampler_cfg
        if roi_sampler_cfg['CLS_SCORE_TYPE'] not in _SCORE_TYPES:
            raise NotImplementedError("CLS_SCORE_TYPE %r" % (roi_sampler_cfg['CLS_SCORE_TYPE'],))

    def forward(self, batch_dict, seed=None, draws=None, check=False):
        """batch_dict: batch_size, rois (B, M, 7), roi_scores (B, M), roi_labels (B, M) int64, gt_boxes (B, T, 8).
        Returns the reference's targets_dict -- rois (B, R, 7), gt_of_rois (B, R, 8), gt_iou_of_rois, roi_scores,
        roi_labels, reg_valid_mask (int64), rcnn_cls_labels (int64 for 'cls', float32 for 'roi_iou'), R = ROI_PER_IMAGE --
        with gt_of_rois already in each RoI's canonical frame and gt_of_rois_src the untransformed rows, plus
        sampled_inds and status.  check=True reads status once and raises as the reference does for a scene with
        neither foreground nor background; check=False reads nothing."""
        cfg = self.roi_sampler_cfg
        rois, gt = batch_dict['rois'], batch_dict['gt_boxes']
        labels = batch_dict['roi_labels']
        with torch.no_grad():
            max_overlaps, gt_assignment = roi_max_iou(rois, labels, gt, by_class=cfg.get('SAMPLE_ROI_BY_EACH_CLASS', False))
            targets = roi_sample_targets(rois, batch_dict['roi_scores'], labels, gt, max_overlaps, gt_assignment, cfg,
                                         seed=seed, draws=draws)
        if check:
            status = targets['status'].tolist()                 # the one read
            if 1 in status:
                raise NotImplementedError("ERROR: FG=0, BG=0 in scene %d" % status.index(1))
            if 2 in status:
                raise ValueError("a draw or a GT assignment of scene %d is out of range" % status.index(2))
        return targets
