"""PointIntraPartOffsetHead (pcdet/models/dense_heads/point_intra_part_head.py), the point head of Part-A2: a foreground score
and an intra-object part location from every voxel centre UNetV2 returns, under the reference's module names (cls_layers,
part_reg_layers) and state-dict keys.

The reference's assign_stack_targets(ret_part_labels=True) loops over the scenes with boolean masks -- a host read per scene --
and calls points_in_boxes_gpu twice each; its get_part_layer_loss reads the number of foreground points back with .item().
Here both are one entry point of csrc/parta2.hip each and nothing is read on the host:

  part_assign_targets  labels and part labels of a RAGGED stacked point set (any number of rows per scene, any order) in one
                       launch.  PointHeadTemplate.assign_stack_targets needs equally many rows per scene and refuses
                       ret_part_labels; it stays as it is.
  part_loss            get_part_layer_loss with its logit gradient: float64 sums in one fixed order, the number of foreground
                       points kept on the device.  The labels are taken as they are (the reference's binary_cross_entropy
                       device-asserts for a label a hair outside [0, 1]).

As in point_head.py the tb_dict values stay 0-dim device tensors where the reference calls .item().  TARGET_CONFIG.BOX_CODER
(the box branch of the anchor-free PartA2_free.yaml) is refused: none of the configurations built here sets it."""
import ctypes

import torch

from .point_head import PointHeadTemplate
from .pointnet2_batch_cuda import F32, _call, _chk, _partials


def part_assign_targets(points, gt_boxes, extra_width=(0.0, 0.0, 0.0), single_class=True):
    """points (P, 4) float32 [bs_idx, x, y, z], gt_boxes (B, T, 8) float32 -> (labels (P) int64: 0 background, -1 inside an
    enlarged box only, else 1 (single_class) or the box's class; part_labels (P, 3) float32: the point's place in its box in
    [0, 1]^3, zeros where the label is not positive).  One launch, no host read."""
    if points.dim() != 2 or points.shape[1] != 4:
        raise ValueError("points must be (P, 4) [bs_idx, x, y, z], got %s" % (tuple(points.shape),))
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 8 or gt_boxes.shape[0] < 1:
        raise ValueError("gt_boxes must be (B, T, 8) with B >= 1, got %s" % (tuple(gt_boxes.shape),))
    if len(extra_width) != 3:
        raise ValueError("extra_width holds three numbers, got %r" % (extra_width,))
    _chk(points, "points", F32)
    _chk(gt_boxes, "gt_boxes", F32)
    P, (B, T) = points.shape[0], gt_boxes.shape[:2]
    labels = torch.empty((P,), dtype=torch.int64, device=points.device)
    part = torch.empty((P, 3), dtype=F32, device=points.device)
    if P:
        extra = (ctypes.c_float * 3)(*[float(v) for v in extra_width])
        _call("pda_part_assign_targets", points, points.data_ptr(), gt_boxes.data_ptr(), extra, labels.data_ptr(), part.data_ptr(),
              P, B, T, int(bool(single_class)))
    return labels, part


class _PartLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, part_labels, labels, weight):
        P = logits.shape[0]
        out = torch.empty((3,), dtype=F32, device=logits.device)
        grad = torch.empty_like(logits)
        partials = _partials("pda_part_loss_blocks", P, logits.device)
        _call("pda_part_loss", logits, logits.data_ptr(), part_labels.data_ptr(), labels.data_ptr(), float(weight), grad.data_ptr(),
              partials.data_ptr(), out.data_ptr(), P)
        ctx.save_for_backward(grad, out)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, grad_loss, _grad_out):
        grad, out = ctx.saved_tensors
        return grad * (out[1] * grad_loss.to(F32)), None, None, None


def part_loss(point_part_preds, point_part_labels, point_cls_labels, weight=1.0):
    """get_part_layer_loss: logits (P, 3), part labels (P, 3), labels (P) int64 -> (loss, out) with out = [loss, weight / (3 *
    max(1, #pos)), #pos] on the device; loss = out[0] is differentiable in the logits."""
    if point_part_preds.dim() != 2 or point_part_preds.shape[1] != 3 or tuple(point_part_labels.shape) != tuple(point_part_preds.shape) \
            or tuple(point_cls_labels.shape) != (point_part_preds.shape[0],):
        raise ValueError("part loss takes logits (P, 3), part labels (P, 3) and labels (P), got %s, %s, %s"
                         % (tuple(point_part_preds.shape), tuple(point_part_labels.shape), tuple(point_cls_labels.shape)))
    logits = point_part_preds.contiguous()
    _chk(logits, "point_part_preds", F32)
    _chk(point_part_labels, "point_part_labels", F32)
    _chk(point_cls_labels, "point_cls_labels", torch.int64)
    return _PartLoss.apply(logits, point_part_labels, point_cls_labels, weight)


class PointIntraPartOffsetHead(PointHeadTemplate):
    """Point-based head for the intra-object part locations (Shi et al., "From Points to Parts", arXiv 1907.03670)."""

    def __init__(self, num_class, input_channels, model_cfg, predict_boxes_when_training=False, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        self.predict_boxes_when_training = predict_boxes_when_training
        if model_cfg['TARGET_CONFIG'].get('BOX_CODER', None) is not None:
            raise NotImplementedError("PointIntraPartOffsetHead with TARGET_CONFIG.BOX_CODER (the box branch of the anchor-free "
                                      "PartA2_free.yaml) is not implemented")
        self.cls_layers = self.make_fc_layers(fc_cfg=model_cfg['CLS_FC'], input_channels=input_channels, output_channels=num_class)
        self.part_reg_layers = self.make_fc_layers(fc_cfg=model_cfg['PART_FC'], input_channels=input_channels, output_channels=3)
        self.box_layers = None

    def assign_targets(self, input_dict):
        """point_coords (N1 + N2 + ..., 4) [bs_idx, x, y, z], gt_boxes (B, M, 8) -> point_cls_labels (N1 + N2 + ...) int64
        (0 background, -1 ignored) and point_part_labels (N1 + N2 + ..., 3)."""
        point_coords = input_dict['point_coords']
        gt_boxes = input_dict['gt_boxes']
        assert gt_boxes.dim() == 3, 'gt_boxes.shape=%s' % str(gt_boxes.shape)
        assert point_coords.dim() == 2, 'points.shape=%s' % str(point_coords.shape)
        labels, part = part_assign_targets(point_coords.detach().float().contiguous(), gt_boxes.detach().float().contiguous(),
                                           self.model_cfg['TARGET_CONFIG']['GT_EXTRA_WIDTH'], self.num_class == 1)
        return {'point_cls_labels': labels, 'point_part_labels': part, 'point_box_labels': None}

    def get_part_layer_loss(self, tb_dict=None):
        ret = self.forward_ret_dict
        weight = self.model_cfg['LOSS_CONFIG']['LOSS_WEIGHTS']['point_part_weight']
        point_loss_part, _ = part_loss(ret['point_part_preds'], ret['point_part_labels'], ret['point_cls_labels'], weight)
        if tb_dict is None:
            tb_dict = {}
        tb_dict.update({'point_loss_part': point_loss_part.detach()})
        return point_loss_part, tb_dict

    def get_loss(self, tb_dict=None):
        tb_dict = {} if tb_dict is None else tb_dict
        point_loss_cls, tb_dict_1 = self.get_cls_layer_loss()
        point_loss_part, tb_dict_2 = self.get_part_layer_loss()
        tb_dict.update(tb_dict_1)
        tb_dict.update(tb_dict_2)
        return point_loss_cls + point_loss_part, tb_dict

    def forward(self, batch_dict):
        """point_features (N1 + N2 + ..., C), point_coords (N1 + N2 + ..., 4) -> point_cls_scores (N1 + N2 + ...) and
        point_part_offset (N1 + N2 + ..., 3), both after the sigmoid."""
        point_features = batch_dict['point_features']
        point_cls_preds = self.cls_layers(point_features)                       # (total_points, num_class)
        point_part_preds = self.part_reg_layers(point_features)
        ret_dict = {'point_cls_preds': point_cls_preds, 'point_part_preds': point_part_preds}
        point_cls_scores = torch.sigmoid(point_cls_preds)
        batch_dict['point_cls_scores'], _ = point_cls_scores.max(dim=-1)
        batch_dict['point_part_offset'] = torch.sigmoid(point_part_preds)
        if self.training:
            targets_dict = self.assign_targets(batch_dict)
            ret_dict['point_cls_labels'] = targets_dict['point_cls_labels']
            ret_dict['point_part_labels'] = targets_dict['point_part_labels']
            ret_dict['point_box_labels'] = None
        self.forward_ret_dict = ret_dict
        return batch_dict
