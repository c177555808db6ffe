"""The operators behind CenterHead on the device (csrc/center_head.hip): what the reference builds from
pcdet/models/model_utils/centernet_utils.py (gaussian_radius, draw_gaussian_to_heatmap, _topk, decode_bbox_from_heatmap)
and pcdet/utils/loss_utils.py:395-517 (neg_loss_cornernet, _reg_loss).  None of them reads anything back to the host, so
target assignment, both losses and their backward replay from one captured graph.

center_targets     CenterHead.assign_targets for the batch and all heads, one launch.
focal_loss         FocalLossCenterNet on the LOGITS (the clamped sigmoid is evaluated inside), one pass + one small launch.
reg_loss           RegLossCenterNet over the HEAD_ORDER maps as they are (no cat, no channel-last copy), one launch.
decode_topk        decode_bbox_from_heatmap behind one library topk on the logits, one launch.

Departures from the reference, all in DESIGN.md: gt_boxes is not written (the reference re-labels the caller's tensor in
place); a regression target that is NaN contributes 0 (the reference's 0 * NaN turns the whole column into NaN); ties
among heat-map scores, which the reference leaves to torch.topk, are outside the parity claim; gaussian2D's eps cut-off
cannot fire and is left out."""
import ctypes

import torch

from .pointnet2_batch_cuda import F32, _call, _chk, _partials, _ptr_array

I64 = torch.int64
MAX_OBJS = 2048           # csrc/center_head.hip CH_MAX_OBJS
MAX_CODE = 16             # CH_MAX_CODE
MAX_HEADS = 8
MAX_CLASSES = 32


class HeadLayout:
    """CLASS_NAMES_EACH_HEAD against class_names as the host arrays pda_center_assign_targets takes: a label (1-based
    index into class_names) -> its head and its index inside the head."""

    def __init__(self, class_names, class_names_each_head):
        self.num_class = len(class_names)
        if not 1 <= self.num_class <= MAX_CLASSES or not 1 <= len(class_names_each_head) <= MAX_HEADS:
            raise ValueError("at most %d classes and %d heads" % (MAX_CLASSES, MAX_HEADS))
        head_of, local_of = [-1] * (self.num_class + 1), [-1] * (self.num_class + 1)
        for h, names in enumerate(class_names_each_head):
            for j, name in enumerate(names):
                label = list(class_names).index(name) + 1
                if head_of[label] < 0:                       # `name in cur_class_names`, first head first
                    head_of[label], local_of[label] = h, j
        self.head_classes = [len(names) for names in class_names_each_head]
        self.n_heads = len(self.head_classes)
        self.head_of_c = (ctypes.c_int32 * len(head_of))(*head_of)
        self.local_of_c = (ctypes.c_int32 * len(local_of))(*local_of)
        self.head_classes_c = (ctypes.c_int32 * self.n_heads)(*self.head_classes)


def center_targets(gt_boxes, layout, feature_map_size, point_cloud_range, voxel_size, feature_map_stride, num_max_objs,
                   gaussian_overlap, min_radius):
    """gt_boxes (B, M, 8 or 10) float32 on the device, zero-padded, the label in the last column; feature_map_size (H, W).
    Returns the reference's ret_dict: per head heatmaps (B, C_h, H, W), target_boxes (B, NUM_MAX_OBJS, code), inds and
    masks (B, NUM_MAX_OBJS) int64.  gt_boxes is not written.  One fill per head and one launch; no host read."""
    _chk(gt_boxes, "gt_boxes", F32)
    if gt_boxes.dim() != 3 or not 8 <= gt_boxes.shape[-1] <= MAX_CODE:
        raise ValueError("gt_boxes must be (B, M, 8..%d), got %s" % (MAX_CODE, tuple(gt_boxes.shape)))
    K = int(num_max_objs)
    if not 1 <= K <= MAX_OBJS:
        raise ValueError("NUM_MAX_OBJS must lie in 1..%d, got %d" % (MAX_OBJS, K))
    B, M, cols = gt_boxes.shape
    H, W = (int(v) for v in feature_map_size)
    dev = gt_boxes.device
    ret = {'heatmaps': [], 'target_boxes': [], 'inds': [], 'masks': [], 'heatmap_masks': []}
    for c in layout.head_classes:
        ret['heatmaps'].append(torch.zeros((B, c, H, W), dtype=F32, device=dev))
        ret['target_boxes'].append(torch.empty((B, K, cols), dtype=F32, device=dev))
        ret['inds'].append(torch.empty((B, K), dtype=I64, device=dev))
        ret['masks'].append(torch.empty((B, K), dtype=I64, device=dev))
    if B == 0 or H == 0 or W == 0:
        for key in ('target_boxes', 'inds', 'masks'):
            for t in ret[key]:
                t.zero_()
        return ret
    _call("pda_center_assign_targets", gt_boxes, gt_boxes.data_ptr(), cols, B, M, layout.num_class, layout.n_heads,
          layout.head_of_c, layout.local_of_c, layout.head_classes_c, H, W, K, float(point_cloud_range[0]),
          float(point_cloud_range[1]), float(voxel_size[0]), float(voxel_size[1]), float(feature_map_stride),
          float(gaussian_overlap), int(min_radius), _ptr_array(ret['heatmaps']), _ptr_array(ret['target_boxes']),
          _ptr_array(ret['inds']), _ptr_array(ret['masks']))
    return ret


class _FocalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, heatmap, weight):
        n = logits.numel()
        out = torch.zeros((3,), dtype=F32, device=logits.device)
        grad = torch.empty_like(logits)
        if n:
            partials = _partials("pda_center_focal_blocks", n, logits.device)
            _call("pda_center_focal_loss", logits, _chk(logits, "logits", F32), _chk(heatmap, "heatmap", F32), n, grad.data_ptr(),
                  partials.data_ptr(), out.data_ptr())
        else:
            out[1] = -1.0
        ctx.save_for_backward(grad, out)
        ctx.weight = weight
        return out[0] * weight if weight != 1.0 else out[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        g, out = ctx.saved_tensors
        res = torch.empty_like(g)
        go = grad_out.contiguous().to(F32)
        _call("pda_center_scale", g, g.data_ptr(), out[1:2].data_ptr(), go.data_ptr(), ctx.weight, g.numel(), res.data_ptr())
        return res, None, None


def focal_loss(logits, heatmap, weight=1.0):
    """FocalLossCenterNet()(clamp(sigmoid(logits), 1e-4, 1 - 1e-4), heatmap) * weight as a 0-dim device tensor,
    differentiable in logits (any shape, contiguous).  The derivative is zero where the clamp is active.  The reference's
    branch on num_pos == 0 is taken on the device."""
    if logits.shape != heatmap.shape:
        raise ValueError("logits %s and heatmap %s differ in shape" % (tuple(logits.shape), tuple(heatmap.shape)))
    _chk(heatmap, "heatmap", F32)
    return _FocalLoss.apply(logits.contiguous(), heatmap, float(weight))


class _RegLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, targets, inds, masks, code_weights, loc_weight, *maps):
        B, K, code = targets.shape
        hw = maps[0].shape[2] * maps[0].shape[3]
        channels = [m.shape[1] for m in maps]
        ch_c = (ctypes.c_int32 * len(maps))(*channels)
        w_c = (ctypes.c_float * code)(*[float(w) for w in code_weights])
        out = torch.zeros((2 + code,), dtype=F32, device=targets.device)
        if B * K:
            _call("pda_center_reg_loss", targets, _ptr_array(maps), ch_c, len(maps), targets.data_ptr(), inds.data_ptr(),
                  masks.data_ptr(), w_c, float(loc_weight), B, K, hw, out.data_ptr())
        else:
            out[1] = 1.0
        ctx.save_for_backward(targets, inds, masks, out, *maps)
        ctx.host = (ch_c, w_c, float(loc_weight), B, K, hw)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, grad_loss, _grad_out):
        targets, inds, masks, out = ctx.saved_tensors[:4]
        maps = ctx.saved_tensors[4:]
        ch_c, w_c, loc_weight, B, K, hw = ctx.host
        grads = [torch.zeros_like(m) for m in maps]
        if B * K and hw:
            go = grad_loss.contiguous().to(F32)
            _call("pda_center_reg_loss_grad", targets, _ptr_array(maps), ch_c, len(maps), targets.data_ptr(), inds.data_ptr(),
                  masks.data_ptr(), w_c, loc_weight, B, K, hw, out.data_ptr(), go.data_ptr(), _ptr_array(grads))
        return (None, None, None, None, None) + tuple(grads)


def reg_loss(maps, masks, inds, targets, code_weights, loc_weight=1.0):
    """maps: the HEAD_ORDER predictions, each (B, c_i, H, W) float32; masks, inds (B, K) int64; targets (B, K, sum c_i).
    Returns (loc_loss, detail): loc_loss = sum(RegLossCenterNet(cat(maps), masks, inds, targets) * code_weights) *
    loc_weight as a 0-dim tensor, differentiable in the maps; detail = [loc_loss, max(sum(mask), 1), the code columns]."""
    maps = [m.contiguous() for m in maps]
    for m in maps:
        _chk(m, "map", F32)
        if m.dim() != 4 or m.shape[0] != targets.shape[0] or m.shape[2:] != maps[0].shape[2:]:
            raise ValueError("the maps must be (B, c, H, W) with one B, H and W")
    code = sum(m.shape[1] for m in maps)
    if targets.dim() != 3 or targets.shape[2] != code or code > MAX_CODE or len(code_weights) != code:
        raise ValueError("targets %s and %d code weights do not fit maps of %d channels (at most %d)"
                         % (tuple(targets.shape), len(code_weights), code, MAX_CODE))
    if masks.shape != targets.shape[:2] or inds.shape != targets.shape[:2]:
        raise ValueError("masks and inds must be (B, K)")
    _chk(targets, "targets", F32), _chk(inds, "inds", I64), _chk(masks, "masks", I64)
    return _RegLoss.apply(targets, inds, masks, tuple(code_weights), loc_weight, *maps)


def decode_topk(pred_dict, K, class_map, point_cloud_range, voxel_size, feature_map_stride, post_center_limit_range,
                score_thresh=None):
    """pred_dict: one head's maps 'hm' (B, C, H, W) LOGITS, 'center', 'center_z', 'dim', 'rot' and optionally 'vel'.
    Among distinct scores the reference's two-stage _topk equals the top K of the flattened (C * H * W) map, and the
    sigmoid is monotonic: one library topk on the logits selects, the sigmoid is applied to the K selected values.
    Returns boxes (B, K, 7 or 9), scores (B, K) (-inf for a row outside post_center_limit_range or not above score_thresh)
    and labels (B, K) int64 = class_map[class] (0-based, as class_id_mapping_each_head)."""
    hm = pred_dict['hm']
    _chk(hm.contiguous(), "hm", F32)
    B, C, H, W = hm.shape
    K = min(int(K), C * H * W)
    vel = pred_dict.get('vel')
    boxes = torch.empty((B, K, 9 if vel is not None else 7), dtype=F32, device=hm.device)
    scores = torch.empty((B, K), dtype=F32, device=hm.device)
    labels = torch.empty((B, K), dtype=I64, device=hm.device)
    if B * K == 0:
        return boxes, scores, labels
    top, ind = torch.topk(hm.detach().reshape(B, -1), K)
    maps = [pred_dict[k].detach().contiguous() for k in ('center', 'center_z', 'dim', 'rot')]
    for m, c in zip(maps, (2, 1, 3, 2)):
        if tuple(m.shape) != (B, c, H, W):
            raise ValueError("a head map has shape %s, expected %s" % (tuple(m.shape), (B, c, H, W)))
        _chk(m, "map", F32)
    velp = None
    if vel is not None:
        vel = vel.detach().contiguous()
        if tuple(vel.shape) != (B, 2, H, W):
            raise ValueError("vel has shape %s" % (tuple(vel.shape),))
        velp = _chk(vel, "vel", F32)
    cm = (ctypes.c_int32 * C)(*[int(v) for v in class_map])
    lim = (ctypes.c_float * 6)(*[float(v) for v in post_center_limit_range])
    _call("pda_center_decode", hm, top.data_ptr(), ind.data_ptr(), *[m.data_ptr() for m in maps], velp, B, K, H, W, C, cm,
          float(feature_map_stride), float(voxel_size[0]), float(voxel_size[1]), float(point_cloud_range[0]),
          float(point_cloud_range[1]), lim, int(score_thresh is not None), float(score_thresh or 0.0), boxes.data_ptr(),
          scores.data_ptr(), labels.data_ptr())
    return boxes, scores, labels
