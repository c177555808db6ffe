"""The anchor head of PointPillar, SECOND, PartA2, PV-RCNN and Voxel-RCNN on the device (pcdet/models/dense_heads/
anchor_head_template.py, anchor_head_single.py, target_assigner/anchor_generator.py, axis_aligned_target_assigner.py) under
the reference's class names, constructor signatures, config keys and state-dict keys (conv_cls, conv_box, conv_dir_cls).
The 1x1 convolutions stay in torch; target assignment, the three losses and the box decoding are csrc/anchor_head.hip
(pda_anchor_*): two launches for the targets of the whole batch and all anchor classes, one pass and one small finishing
launch for the losses, one launch for the decoding.  Nothing is read back to the host, so forward + get_loss + backward
replay from one captured graph.

`self.anchors` is built on the host exactly as the reference builds it (float32 arange, meshgrid, permute(2, 1, 0, 3, 4, 5),
z += dz / 2), so the tensors are bit-identical; they are uploaded once as one (N, 7) table in the order of the targets.

Departures from the reference: tb_dict holds 0-dim device tensors; box_cls_labels is not rewritten
for num_class == 1; a gt row with label 0 takes part in no class (the reference maps it onto the last class, where its zero
area can influence nothing).  Out of contract, raised as NotImplementedError: POS_FRACTION >= 0, NORM_BY_NUM_EXAMPLES,
MATCH_HEIGHT, NAME: ATSS, boxes with more than 7 + 1 columns, encode_angle_by_sincos, and on AnchorHeadSingle USE_MULTIHEAD
and anchor classes with different feature_map_stride (anchor_head_multi.py has the head of USE_MULTIHEAD)."""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import box_coder_utils
from .config import field
from .pointnet2_batch_cuda import F32, I32, _call, _chk, _partials

MAX_CLASSES = 32          # csrc/anchor_head.hip AH_MAX_CLASSES
MAX_SLOTS = 64            # AH_MAX_SLOTS
MAX_BINS = 8              # AH_MAX_BINS


class AnchorGenerator(object):
    def __init__(self, anchor_range, anchor_generator_config):
        self.anchor_generator_cfg = anchor_generator_config
        self.anchor_range = anchor_range
        self.anchor_sizes = [config['anchor_sizes'] for config in anchor_generator_config]
        self.anchor_rotations = [config['anchor_rotations'] for config in anchor_generator_config]
        self.anchor_heights = [config['anchor_bottom_heights'] for config in anchor_generator_config]
        self.align_center = [field(config, 'align_center', False) for config in anchor_generator_config]
        assert len(self.anchor_sizes) == len(self.anchor_rotations) == len(self.anchor_heights)
        self.num_of_anchor_sets = len(self.anchor_sizes)

    def generate_anchors(self, grid_sizes):
        """Per anchor class a HOST tensor (nz, ny, nx, n_sizes, n_rotations, 7) and the anchors per location, every value the
        bits of the reference's (anchor_generator.py:17-60): the same float32 operations in the same order."""
        assert len(grid_sizes) == self.num_of_anchor_sets
        all_anchors, num_anchors_per_location = [], []
        r = self.anchor_range
        for grid_size, sizes, rotations, heights, align_center in zip(grid_sizes, self.anchor_sizes, self.anchor_rotations,
                                                                      self.anchor_heights, self.align_center):
            num_anchors_per_location.append(len(rotations) * len(sizes) * len(heights))
            if align_center:
                x_stride, y_stride = (r[3] - r[0]) / grid_size[0], (r[4] - r[1]) / grid_size[1]
                x_offset, y_offset = x_stride / 2, y_stride / 2
            else:
                x_stride, y_stride = (r[3] - r[0]) / (grid_size[0] - 1), (r[4] - r[1]) / (grid_size[1] - 1)
                x_offset, y_offset = 0, 0
            x_shifts = torch.arange(r[0] + x_offset, r[3] + 1e-5, step=x_stride, dtype=torch.float32)
            y_shifts = torch.arange(r[1] + y_offset, r[4] + 1e-5, step=y_stride, dtype=torch.float32)
            z_shifts = x_shifts.new_tensor(heights)
            n_size, n_rot = len(sizes), len(rotations)
            rot = x_shifts.new_tensor(rotations)
            size = x_shifts.new_tensor(sizes)
            xs, ys, zs = torch.meshgrid([x_shifts, y_shifts, z_shifts], indexing='ij')
            anchors = torch.stack((xs, ys, zs), dim=-1)
            anchors = anchors[:, :, :, None, :].repeat(1, 1, 1, n_size, 1)
            size = size.view(1, 1, 1, -1, 3).repeat([*anchors.shape[0:3], 1, 1])
            anchors = torch.cat((anchors, size), dim=-1)
            anchors = anchors[:, :, :, :, None, :].repeat(1, 1, 1, 1, n_rot, 1)
            rot = rot.view(1, 1, 1, 1, -1, 1).repeat([*anchors.shape[0:3], n_size, 1, 1])
            anchors = torch.cat((anchors, rot), dim=-1)
            anchors = anchors.permute(2, 1, 0, 3, 4, 5).contiguous()
            anchors[..., 2] += anchors[..., 5] / 2
            all_anchors.append(anchors)
        return all_anchors, num_anchors_per_location


def anchor_table(anchors):
    """The per-class anchors (nz, ny, nx, n_sizes, n_rot, 7) -> one (N, 7) table in the order of the targets: the reference's
    cat over the per-class (nz, ny, nx, A_c) tensors along the last axis.  Returns the table and A_c per class."""
    lead = anchors[0].shape[:3]
    if any(a.shape[:3] != lead for a in anchors):
        raise NotImplementedError("anchor classes with different feature_map_stride (the reference's torch.cat fails there)")
    if any(a.shape[4] != anchors[0].shape[4] for a in anchors):
        raise NotImplementedError("anchor classes with different numbers of rotations (the reference's torch.cat fails there)")
    flat = [a.reshape(*lead, -1, 7) for a in anchors]
    return torch.cat(flat, dim=-2).reshape(-1, 7).contiguous(), [f.shape[3] for f in flat]


class AxisAlignedTargetAssigner(object):
    CLASS_MAJOR = False       # anchor_head_multi.ClassMajorTargetAssigner: the table of USE_MULTIHEAD
    CODED = False             # anchor_head_coded: sin-cos headings and custom columns
    ENTRY = "pda_anchor_assign_targets"

    def __init__(self, model_cfg, class_names, box_coder, match_height=False):
        generator_cfg = model_cfg['ANCHOR_GENERATOR_CONFIG']
        target_cfg = model_cfg['TARGET_ASSIGNER_CONFIG']
        self.box_coder = box_coder
        self.match_height = match_height
        self.class_names = np.array(class_names)
        self.anchor_class_names = [config['class_name'] for config in generator_cfg]
        if target_cfg['POS_FRACTION'] >= 0:
            raise NotImplementedError("POS_FRACTION >= 0 (no yaml of the reference uses it; its sampling indexes labels with "
                                      "positions of fg_inds)")
        if target_cfg['NORM_BY_NUM_EXAMPLES']:
            raise NotImplementedError("NORM_BY_NUM_EXAMPLES: True")
        if match_height:
            raise NotImplementedError("MATCH_HEIGHT: True (rotated 3D IoU matching)")
        if bool(field(model_cfg, 'USE_MULTIHEAD', False)) != self.CLASS_MAJOR:
            raise NotImplementedError("USE_MULTIHEAD: %s (anchor_head_multi.AnchorHeadMulti has the class-major assigner)"
                                      % field(model_cfg, 'USE_MULTIHEAD', False))
        if not self.CODED and (getattr(box_coder, 'encode_angle_by_sincos', False) or box_coder.code_size != 7):
            raise NotImplementedError("encode_angle_by_sincos / a code size other than 7 (anchor_head_coded has them)")
        self.pos_fraction = None
        self.sample_size = target_cfg['SAMPLE_SIZE']
        self.norm_by_num_examples = False
        self.matched_thresholds = {c['class_name']: c['matched_threshold'] for c in generator_cfg}
        self.unmatched_thresholds = {c['class_name']: c['unmatched_threshold'] for c in generator_cfg}
        self.use_multihead = self.CLASS_MAJOR
        names = self.anchor_class_names
        if not 1 <= len(names) <= MAX_CLASSES or len(set(names)) != len(names):
            raise ValueError("1..%d anchor classes with different names, got %s" % (MAX_CLASSES, names))
        labels = [list(class_names).index(n) + 1 for n in names]
        self._label_c = (ctypes.c_int32 * len(names))(*labels)
        self._matched_c = (ctypes.c_float * len(names))(*[float(self.matched_thresholds[n]) for n in names])
        self._unmatched_c = (ctypes.c_float * len(names))(*[float(self.unmatched_thresholds[n]) for n in names])
        self._table = {}

    def build_table(self, anchors):
        """The host table of the per-class anchors and what each class owns of it: here its slots at every location."""
        tab, counts = anchor_table(anchors)
        if sum(counts) > MAX_SLOTS:
            raise ValueError("at most %d anchors per location, got %d" % (MAX_SLOTS, sum(counts)))
        return tab, counts

    def table(self, all_anchors, device):
        """The (N, 7) device table of `all_anchors` (the head's list) and the per-class slot counts, uploaded once."""
        key = (id(all_anchors), str(device))
        hit = self._table.get(key)
        if hit is None:
            tab, counts = self.build_table([a.detach().cpu() for a in all_anchors])
            hit = self._table[key] = (tab.to(device), (ctypes.c_int32 * len(counts))(*counts), all_anchors)
        return hit[0], hit[1]

    def assign_targets(self, all_anchors, gt_boxes_with_classes):
        """all_anchors: the head's per-class anchors; gt_boxes (B, M, 8) float32 on the device, zero-padded, the 1-based label
        last.  Returns box_cls_labels (B, N) int32, box_reg_targets (B, N, 7), reg_weights (B, N) and num_pos (B) int32 (the
        positives of each scene, which the loss needs).  Two launches; no host read; gt_boxes is not written."""
        gt = gt_boxes_with_classes
        if not isinstance(gt, torch.Tensor) or gt.dim() != 3:
            raise ValueError("gt_boxes must be a (B, M, 8) tensor")
        if gt.shape[-1] != 8:
            raise NotImplementedError("gt_boxes with %d columns: boxes with more than 7 + 1 columns are out of contract"
                                      % gt.shape[-1])
        _chk(gt, "gt_boxes", F32)
        B, M = gt.shape[0], gt.shape[1]
        table, counts = self.table(all_anchors, gt.device)
        N = table.shape[0]
        dev = gt.device
        labels = torch.empty((B, N), dtype=I32, device=dev)
        targets = torch.empty((B, N, 7), dtype=F32, device=dev)
        weights = torch.empty((B, N), dtype=F32, device=dev)
        num_pos = torch.empty((B,), dtype=I32, device=dev)
        col_max = torch.empty((B, max(M, 1)), dtype=I32, device=dev)
        if B and N:
            _call(self.ENTRY, gt, gt.data_ptr(), 8, B, M, table.data_ptr(), N, len(self.anchor_class_names),
                  self._label_c, self._matched_c, self._unmatched_c, counts, col_max.data_ptr(), labels.data_ptr(),
                  targets.data_ptr(), weights.data_ptr(), num_pos.data_ptr())
        return {'box_cls_labels': labels, 'box_reg_targets': targets, 'reg_weights': weights, 'num_pos': num_pos}


_ONE = {}


def _one(dev):
    key = str(dev)
    if key not in _ONE:
        _ONE[key] = torch.ones((1,), dtype=F32, device=dev)
    return _ONE[key]


class _AnchorLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cls_preds, box_preds, dir_preds, labels, targets, num_pos, table, host):
        code_w, cls_w, loc_w, dir_w, dir_offset, num_class, bins, *coded = host      # coded: (code, sincos, reg_loss)
        B, N = labels.shape
        dev = cls_preds.device
        out = torch.empty((4,), dtype=F32, device=dev)
        g_cls, g_box = torch.empty_like(cls_preds), torch.empty_like(box_preds)
        g_dir = torch.empty_like(dir_preds) if dir_preds is not None else None
        partials = _partials("pda_anchor_loss_blocks", B * N, dev)
        _call("pda_anchor_loss_coded" if coded else "pda_anchor_loss", cls_preds, *coded, cls_preds.data_ptr(), box_preds.data_ptr(),
              None if dir_preds is None else dir_preds.data_ptr(), labels.data_ptr(), targets.data_ptr(), num_pos.data_ptr(),
              table.data_ptr(), B, N, num_class, bins, code_w, cls_w, loc_w, dir_w, dir_offset, g_cls.data_ptr(),
              g_box.data_ptr(), None if g_dir is None else g_dir.data_ptr(), partials.data_ptr(), out.data_ptr())
        ctx.grads = (g_cls, g_box, g_dir)
        ctx.mark_non_differentiable(out)
        return out[3].clone(), out

    @staticmethod
    def backward(ctx, grad_loss, _grad_out):
        go = grad_loss.contiguous().to(F32).reshape(1)
        one = _one(go.device)
        res = []
        for g in ctx.grads:
            if g is None:
                res.append(None)
                continue
            r = torch.empty_like(g)
            _call("pda_center_scale", g, g.data_ptr(), go.data_ptr(), one.data_ptr(), 1.0, g.numel(), r.data_ptr())
            res.append(r)
        return res[0], res[1], res[2], None, None, None, None, None


def anchor_loss(cls_preds, box_preds, dir_cls_preds, box_cls_labels, box_reg_targets, num_pos, table, num_class, code_weights,
                cls_weight, loc_weight, dir_weight=0.0, dir_offset=0.0):
    """The fused get_cls_layer_loss + get_box_reg_layer_loss.  cls_preds (B, N, num_class), box_preds (B, N, 7),
    dir_cls_preds (B, N, bins) or None; labels (B, N) int32, targets (B, N, 7), num_pos (B) int32 from assign_targets; table
    (N, 7) the anchors.  Returns (rpn_loss, out) with out = [rpn_loss_cls, rpn_loss_loc, rpn_loss_dir, rpn_loss] on the
    device; rpn_loss is differentiable in the three predictions."""
    B, N = box_cls_labels.shape
    preds = [cls_preds.reshape(B, N, -1).contiguous(), box_preds.reshape(B, N, -1).contiguous(),
             None if dir_cls_preds is None else dir_cls_preds.reshape(B, N, -1).contiguous()]
    for name, t in zip(("cls_preds", "box_preds", "dir_cls_preds"), preds):
        if t is not None:
            _chk(t, name, F32)
    _chk(box_cls_labels, "box_cls_labels", I32), _chk(box_reg_targets, "box_reg_targets", F32), _chk(num_pos, "num_pos", I32)
    _chk(table, "anchors", F32)
    if preds[0].shape[2] != num_class or not 1 <= num_class <= MAX_CLASSES:
        raise ValueError("cls_preds %s do not hold %d classes (at most %d)" % (tuple(cls_preds.shape), num_class, MAX_CLASSES))
    if preds[1].shape[2] != 7 or tuple(box_reg_targets.shape) != (B, N, 7) or table.shape != (N, 7) or num_pos.numel() != B:
        raise ValueError("box_preds, box_reg_targets, anchors and num_pos must be (B, N, 7), (B, N, 7), (N, 7) and (B)")
    if len(code_weights) != 7:
        raise NotImplementedError("%d code weights: boxes with more than 7 columns are out of contract" % len(code_weights))
    bins = 0 if preds[2] is None else preds[2].shape[2]
    if bins > MAX_BINS:
        raise ValueError("at most %d direction bins, got %d" % (MAX_BINS, bins))
    if B * N == 0:
        raise ValueError("an empty batch has no loss")
    host = ((ctypes.c_float * 7)(*[float(w) for w in code_weights]), float(cls_weight), float(loc_weight), float(dir_weight),
            float(dir_offset), int(num_class), int(bins))
    return _AnchorLoss.apply(preds[0], preds[1], preds[2], box_cls_labels, box_reg_targets, num_pos, table, host)


@torch.no_grad()
def anchor_decode(box_preds, dir_cls_preds, table, dir_offset=0.0, dir_limit_offset=0.0):
    """box_preds (B, N, 7), dir_cls_preds (B, N, bins) or None, table (N, 7) -> batch_box_preds (B, N, 7).  One launch."""
    B, N = box_preds.shape[0], table.shape[0]
    box = box_preds.detach().reshape(B, N, -1).contiguous()
    _chk(box, "box_preds", F32), _chk(table, "anchors", F32)
    if box.shape[2] != 7:
        raise NotImplementedError("box codes with %d columns" % box.shape[2])
    dirs = None
    if dir_cls_preds is not None:
        dirs = dir_cls_preds.detach().reshape(B, N, -1).contiguous()
        _chk(dirs, "dir_cls_preds", F32)
        if dirs.shape[2] > MAX_BINS:
            raise ValueError("at most %d direction bins, got %d" % (MAX_BINS, dirs.shape[2]))
    out = torch.empty((B, N, 7), dtype=F32, device=box.device)
    if B * N:
        _call("pda_anchor_decode", box, box.data_ptr(), None if dirs is None else dirs.data_ptr(), table.data_ptr(), B, N,
              0 if dirs is None else dirs.shape[2], float(dir_offset), float(dir_limit_offset), out.data_ptr())
    return out


class AnchorHeadTemplate(nn.Module):
    MULTIHEAD = False         # anchor_head_multi.AnchorHeadMulti: USE_MULTIHEAD, the class-major table
    CODED = False             # anchor_head_coded: sin-cos headings, custom columns, WeightedL1Loss

    def __init__(self, model_cfg, num_class, class_names, grid_size, point_cloud_range, predict_boxes_when_training):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.class_names = class_names
        self.predict_boxes_when_training = predict_boxes_when_training
        self.use_multihead = field(model_cfg, 'USE_MULTIHEAD', False)
        if bool(self.use_multihead) != self.MULTIHEAD:
            raise NotImplementedError("USE_MULTIHEAD: %s on %s (AnchorHeadMulti is the head of USE_MULTIHEAD: True)"
                                      % (self.use_multihead, type(self).__name__))
        target_cfg = model_cfg['TARGET_ASSIGNER_CONFIG']
        coder = target_cfg['BOX_CODER']
        if coder != 'ResidualCoder':
            raise NotImplementedError("BOX_CODER %r" % (coder,))
        self.box_coder = box_coder_utils.ResidualCoder(num_dir_bins=field(target_cfg, 'NUM_DIR_BINS', 6),
                                                       **(field(target_cfg, 'BOX_CODER_CONFIG', None) or {}))
        if not self.CODED and (self.box_coder.encode_angle_by_sincos or self.box_coder.code_size != 7):
            raise NotImplementedError("encode_angle_by_sincos / boxes with more than 7 columns (anchor_head_coded has them)")
        generator_cfg = model_cfg['ANCHOR_GENERATOR_CONFIG']
        if not self.MULTIHEAD and len({c['feature_map_stride'] for c in generator_cfg}) != 1:
            raise NotImplementedError("anchor classes with different feature_map_stride (the reference's torch.cat fails there)")
        anchors, self.num_anchors_per_location = self.generate_anchors(
            generator_cfg, grid_size=grid_size, point_cloud_range=point_cloud_range,
            anchor_ndim=7 if self.CODED else self.box_coder.code_size)      # coded: the table stays 7 wide, the zero columns implied
        self.anchors = anchors                     # host tensors, the reference's bits; the device table is made once
        self.target_assigner = self.get_target_assigner(target_cfg)
        self.forward_ret_dict = {}
        self.build_losses(model_cfg['LOSS_CONFIG'])

    @staticmethod
    def generate_anchors(anchor_generator_cfg, grid_size, point_cloud_range, anchor_ndim=7):
        generator = AnchorGenerator(anchor_range=point_cloud_range, anchor_generator_config=anchor_generator_cfg)
        grid = np.asarray(grid_size)
        feature_map_size = [grid[:2] // config['feature_map_stride'] for config in anchor_generator_cfg]
        anchors_list, per_location = generator.generate_anchors(feature_map_size)
        if anchor_ndim != 7:
            raise NotImplementedError("anchors with %d columns" % anchor_ndim)
        return anchors_list, per_location

    def get_target_assigner(self, anchor_target_cfg):
        if anchor_target_cfg['NAME'] == 'ATSS':
            raise NotImplementedError("TARGET_ASSIGNER_CONFIG.NAME: ATSS")
        if anchor_target_cfg['NAME'] != 'AxisAlignedTargetAssigner':
            raise NotImplementedError(anchor_target_cfg['NAME'])
        return AxisAlignedTargetAssigner(model_cfg=self.model_cfg, class_names=self.class_names, box_coder=self.box_coder,
                                         match_height=anchor_target_cfg['MATCH_HEIGHT'])

    def build_losses(self, losses_cfg):
        from . import loss_utils
        if field(losses_cfg, 'REG_LOSS_TYPE', None) not in (None, 'WeightedSmoothL1Loss'):
            raise NotImplementedError("REG_LOSS_TYPE %r" % (losses_cfg['REG_LOSS_TYPE'],))
        # the reference's modules, for users of its names; get_loss takes the fused path
        self.add_module('cls_loss_func', loss_utils.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0))
        self.add_module('reg_loss_func', loss_utils.WeightedSmoothL1Loss(code_weights=losses_cfg['LOSS_WEIGHTS']['code_weights']))
        self.add_module('dir_loss_func', loss_utils.WeightedCrossEntropyLoss())

    def anchor_table(self, device):
        return self.target_assigner.table(self.anchors, device)[0]

    def assign_targets(self, gt_boxes):
        """gt_boxes (B, M, 8) -> box_cls_labels, box_reg_targets, reg_weights, num_pos (AxisAlignedTargetAssigner)."""
        with torch.no_grad():
            return self.target_assigner.assign_targets(self.anchors, gt_boxes.contiguous())

    def get_loss(self):
        """(rpn_loss, tb_dict) from forward_ret_dict: one pass over the anchors for the classification, regression and
        direction terms and their gradients.  tb_dict holds 0-dim device tensors under the reference's keys."""
        ret = self.forward_ret_dict
        weights = self.model_cfg['LOSS_CONFIG']['LOSS_WEIGHTS']
        dir_preds = ret.get('dir_cls_preds', None)
        labels = ret['box_cls_labels']
        loss, out = anchor_loss(
            ret['cls_preds'], ret['box_preds'], dir_preds, labels, ret['box_reg_targets'], ret['num_pos'],
            self.anchor_table(labels.device), self.num_class, weights['code_weights'], weights['cls_weight'],
            weights['loc_weight'], weights['dir_weight'] if dir_preds is not None else 0.0,
            self.model_cfg['DIR_OFFSET'] if dir_preds is not None else 0.0)
        tb_dict = {'rpn_loss_cls': out[0], 'rpn_loss_loc': out[1]}
        if dir_preds is not None:
            tb_dict['rpn_loss_dir'] = out[2]
        tb_dict['rpn_loss'] = out[3]
        return loss, tb_dict

    def generate_predicted_boxes(self, batch_size, cls_preds, box_preds, dir_cls_preds=None):
        """cls_preds (B, H, W, A * num_class), box_preds (B, H, W, A * 7), dir_cls_preds (B, H, W, A * bins) or None ->
        batch_cls_preds (B, N, num_class), batch_box_preds (B, N, 7).  One launch."""
        table = self.anchor_table(box_preds.device)
        batch_cls_preds = cls_preds.view(batch_size, table.shape[0], -1).float()
        if dir_cls_preds is not None:
            boxes = anchor_decode(box_preds, dir_cls_preds, table, self.model_cfg['DIR_OFFSET'], self.model_cfg['DIR_LIMIT_OFFSET'])
        else:
            boxes = anchor_decode(box_preds, None, table)
        return batch_cls_preds, boxes

    def forward(self, **kwargs):
        raise NotImplementedError


class AnchorHeadSingle(AnchorHeadTemplate):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range,
                 predict_boxes_when_training=True, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class, class_names=class_names, grid_size=grid_size,
                         point_cloud_range=point_cloud_range, predict_boxes_when_training=predict_boxes_when_training)
        self.num_anchors_per_location = sum(self.num_anchors_per_location)
        self.conv_cls = nn.Conv2d(input_channels, self.num_anchors_per_location * self.num_class, kernel_size=1)
        self.conv_box = nn.Conv2d(input_channels, self.num_anchors_per_location * self.box_coder.code_size, kernel_size=1)
        if field(model_cfg, 'USE_DIRECTION_CLASSIFIER', None) is not None:
            if not 1 <= model_cfg['NUM_DIR_BINS'] <= MAX_BINS:
                raise ValueError("NUM_DIR_BINS must lie in 1..%d" % MAX_BINS)
            self.conv_dir_cls = nn.Conv2d(input_channels, self.num_anchors_per_location * model_cfg['NUM_DIR_BINS'], kernel_size=1)
        else:
            self.conv_dir_cls = None
        self.init_weights()

    def init_weights(self):
        pi = 0.01
        nn.init.constant_(self.conv_cls.bias, -np.log((1 - pi) / pi))
        nn.init.normal_(self.conv_box.weight, mean=0, std=0.001)

    def forward(self, data_dict):
        spatial_features_2d = data_dict['spatial_features_2d']
        cls_preds = self.conv_cls(spatial_features_2d).permute(0, 2, 3, 1).contiguous()      # [N, H, W, C]
        box_preds = self.conv_box(spatial_features_2d).permute(0, 2, 3, 1).contiguous()
        self.forward_ret_dict['cls_preds'] = cls_preds
        self.forward_ret_dict['box_preds'] = box_preds
        if self.conv_dir_cls is not None:
            dir_cls_preds = self.conv_dir_cls(spatial_features_2d).permute(0, 2, 3, 1).contiguous()
            self.forward_ret_dict['dir_cls_preds'] = dir_cls_preds
        else:
            dir_cls_preds = None
        if self.training:
            self.forward_ret_dict.update(self.assign_targets(gt_boxes=data_dict['gt_boxes']))
        if not self.training or self.predict_boxes_when_training:
            batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(
                batch_size=data_dict['batch_size'], cls_preds=cls_preds, box_preds=box_preds, dir_cls_preds=dir_cls_preds)
            data_dict['batch_cls_preds'] = batch_cls_preds
            data_dict['batch_box_preds'] = batch_box_preds
            data_dict['cls_preds_normalized'] = False
        return data_dict
