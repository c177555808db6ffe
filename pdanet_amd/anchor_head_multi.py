"""AnchorHeadMulti and SingleHead (pcdet/models/dense_heads/anchor_head_multi.py), the dense head of
kitti_models/second_multihead.yaml, under the reference's class names, constructor signatures, config keys and state-dict keys
(shared_conv.*, rpn_heads.<i>.conv_cls / conv_box / conv_dir_cls, the head_label_indices buffer, blocks / deblocks where a
head's RPN_HEAD_CFGS entry has LAYER_NUMS).  The convolutions stay in torch.

With USE_MULTIHEAD the anchors of a scene are laid out class after class -- the reference's cat over the classes of
anchors.permute(3, 4, 0, 1, 2, 5).view(-1, 7) -- and head h owns the contiguous rows of its classes.  Target assignment is
pda_anchor_multi_assign_targets (csrc/anchor_head.hip: an anchor's class from the row segment that holds it, so classes may
differ in stride and in their number of rotations); get_cls_layer_loss + get_box_reg_layer_loss are pda_anchor_multi_loss, one
pass and one finishing launch over all heads with the gradients written into per-head tensors; the decoding is
pda_anchor_decode over the class-major table.  Nothing is read back, so forward + get_loss + backward replay from one graph.

Departures from the reference: those of anchor_head.py; RPN_HEAD_CFGS must list the classes in the order
of ANCHOR_GENERATOR_CONFIG (the reference indexes num_anchors_per_location with positions of the concatenated HEAD_CLS_NAME
and silently assumes it): ValueError.  Out of contract, NotImplementedError: what anchor_head.py refuses, USE_MULTIHEAD: False
on this head, and an anchor class with more than one bottom height (the permute(3, 4, 0, ...) view puts the height axis
behind the size and rotation axes, which the heads' (A, H, W) rows do not follow)."""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from .anchor_head import (MAX_BINS, MAX_CLASSES, AnchorHeadTemplate, AxisAlignedTargetAssigner, _one, anchor_decode)
from .base_bev_backbone import BaseBEVBackbone
from .config import field
from .pointnet2_batch_cuda import F32, I32, _call, _chk, _partials, _ptr_array


def class_major_table(anchors):
    """The per-class anchors (nz, ny, nx, n_sizes, n_rot, 7) -> the (N, 7) table of USE_MULTIHEAD and the rows of each class."""
    if any(a.shape[0] != 1 for a in anchors):
        raise NotImplementedError("an anchor class with more than one bottom height under USE_MULTIHEAD")
    flat = [a.permute(3, 4, 0, 1, 2, 5).contiguous().view(-1, a.shape[-1]) for a in anchors]
    return torch.cat(flat, dim=0).contiguous(), [f.shape[0] for f in flat]


class ClassMajorTargetAssigner(AxisAlignedTargetAssigner):
    """AxisAlignedTargetAssigner with use_multihead: the same rule per (scene, class, anchor) over the class-major table."""
    CLASS_MAJOR = True
    ENTRY = "pda_anchor_multi_assign_targets"

    def build_table(self, anchors):
        return class_major_table(anchors)


class _AnchorMultiLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, host, labels, targets, num_pos, table, *preds):
        rows, cols, bases, num_class, bins, code_w, weights, *coded = host      # coded: (code, sincos, reg_loss)
        H = len(rows)
        cls, box, dirs = preds[:H], preds[H:2 * H], preds[2 * H:]
        B, N = labels.shape
        dev = labels.device
        out = torch.empty((4,), dtype=F32, device=dev)
        grads = [torch.empty_like(p) for p in preds]
        partials = _partials("pda_anchor_multi_loss_blocks", B * N, dev)
        i32 = lambda v: (ctypes.c_int32 * H)(*v)
        _call("pda_anchor_multi_loss_coded" if coded else "pda_anchor_multi_loss", labels, *coded, _ptr_array(cls), _ptr_array(box), _ptr_array(dirs) if dirs else None, H, i32(rows),
              i32(cols), i32(bases), labels.data_ptr(), targets.data_ptr(), num_pos.data_ptr(), table.data_ptr(), B, N, num_class,
              bins, code_w, *weights, _ptr_array(grads[:H]), _ptr_array(grads[H:2 * H]),
              _ptr_array(grads[2 * H:]) if dirs else None, partials.data_ptr(), out.data_ptr())
        ctx.grads = grads
        ctx.mark_non_differentiable(out)
        return out[3].clone(), out

    @staticmethod
    def backward(ctx, grad_loss, _grad_out):
        go = grad_loss.contiguous().to(F32).reshape(1)
        one = _one(go.device)
        res = []
        for g in ctx.grads:
            r = torch.empty_like(g)
            _call("pda_center_scale", g, g.data_ptr(), go.data_ptr(), one.data_ptr(), 1.0, g.numel(), r.data_ptr())
            res.append(r)
        return (None, None, None, None, None) + tuple(res)


def anchor_multi_loss(cls_preds, box_preds, dir_cls_preds, head_cols, head_col_base, box_cls_labels, box_reg_targets, num_pos,
                      table, num_class, code_weights, cls_weight, loc_weight, dir_weight=0.0, dir_offset=0.0, pos_cls_weight=1.0,
                      neg_cls_weight=1.0):
    """The fused get_cls_layer_loss + get_box_reg_layer_loss of AnchorHeadMulti over lists of per-head predictions: cls_preds[h]
    (B, N_h, head_cols[h]), box_preds[h] (B, N_h, 7), dir_cls_preds[h] (B, N_h, bins) or dir_cls_preds None; head h owns the N_h
    rows of the class-major table (N, 7) behind those of the heads before it, and a positive of label l is hot at its column
    l - 1 - head_col_base[h].  labels (B, N) int32, targets (B, N, 7), num_pos (B) int32 from assign_targets.  Returns
    (rpn_loss, out) with out = [rpn_loss_cls, rpn_loss_loc, rpn_loss_dir, rpn_loss] on the device; rpn_loss is differentiable
    in every prediction."""
    B, N = box_cls_labels.shape
    H = len(cls_preds)
    if not 1 <= H <= MAX_CLASSES or len(box_preds) != H or len(head_cols) != H or len(head_col_base) != H:
        raise ValueError("1..%d heads with one cls_preds, box_preds, column count and column base each" % MAX_CLASSES)
    if dir_cls_preds is not None and len(dir_cls_preds) != H:
        raise ValueError("dir_cls_preds must hold one tensor per head")
    if len(code_weights) != 7:
        raise NotImplementedError("%d code weights: boxes with more than 7 columns are out of contract" % len(code_weights))
    if B * N == 0:
        raise ValueError("an empty batch has no loss")
    _chk(box_cls_labels, "box_cls_labels", I32), _chk(box_reg_targets, "box_reg_targets", F32), _chk(num_pos, "num_pos", I32)
    _chk(table, "anchors", F32)
    if tuple(box_reg_targets.shape) != (B, N, 7) or tuple(table.shape) != (N, 7) or num_pos.numel() != B:
        raise ValueError("box_reg_targets, anchors and num_pos must be (B, N, 7), (N, 7) and (B)")
    cls, box, dirs, rows = [], [], [], []
    for h in range(H):
        b = box_preds[h].reshape(B, -1, 7).contiguous()
        n_h = b.shape[1]
        c = cls_preds[h].reshape(B, n_h, -1).contiguous()
        _chk(c, "cls_preds[%d]" % h, F32), _chk(b, "box_preds[%d]" % h, F32)
        if c.shape[2] != head_cols[h] or head_col_base[h] < 0 or head_col_base[h] + head_cols[h] > num_class:
            raise ValueError("cls_preds[%d] %s do not hold the columns %d..%d of %d classes"
                             % (h, tuple(cls_preds[h].shape), head_col_base[h], head_col_base[h] + head_cols[h], num_class))
        cls.append(c), box.append(b), rows.append(n_h)
        if dir_cls_preds is not None:
            d = dir_cls_preds[h].reshape(B, n_h, -1).contiguous()
            _chk(d, "dir_cls_preds[%d]" % h, F32)
            dirs.append(d)
    if sum(rows) != N:
        raise ValueError("the heads predict %d rows, the table has %d" % (sum(rows), N))
    bins = dirs[0].shape[2] if dirs else 0
    if bins > MAX_BINS or any(d.shape[2] != bins for d in dirs):
        raise ValueError("every head needs the same 1..%d direction bins" % MAX_BINS)
    host = (rows, [int(v) for v in head_cols], [int(v) for v in head_col_base], int(num_class), int(bins),
            (ctypes.c_float * 7)(*[float(w) for w in code_weights]),
            (float(cls_weight), float(loc_weight), float(dir_weight) if dirs else 0.0, float(dir_offset) if dirs else 0.0,
             float(pos_cls_weight), float(neg_cls_weight)))
    return _AnchorMultiLoss.apply(host, box_cls_labels, box_reg_targets, num_pos, table, *cls, *box, *dirs)


class SingleHead(BaseBEVBackbone):
    def __init__(self, model_cfg, input_channels, num_class, num_anchors_per_location, code_size, rpn_head_cfg=None,
                 head_label_indices=None, separate_reg_config=None):
        super().__init__(rpn_head_cfg, input_channels)
        self.num_anchors_per_location = num_anchors_per_location
        self.num_class = num_class
        self.code_size = code_size
        self.model_cfg = model_cfg
        self.separate_reg_config = separate_reg_config
        self.register_buffer('head_label_indices', head_label_indices)

        def middle(c_in):
            layers = []
            for _ in range(separate_reg_config['NUM_MIDDLE_CONV']):
                c_mid = separate_reg_config['NUM_MIDDLE_FILTER']
                layers += [nn.Conv2d(c_in, c_mid, kernel_size=3, stride=1, padding=1, bias=False), nn.BatchNorm2d(c_mid), nn.ReLU()]
                c_in = c_mid
            return layers, c_in

        if separate_reg_config is not None:
            self.conv_box = nn.ModuleDict()      # registered before conv_cls, as in the reference: the state-dict order
            self.conv_box_names = []
            layers, c_in = middle(input_channels)
            self.conv_cls = nn.Sequential(*layers, nn.Conv2d(c_in, num_anchors_per_location * num_class, kernel_size=3, stride=1,
                                                             padding=1))
            code_size_cnt = 0
            for reg_config in separate_reg_config['REG_LIST']:
                reg_name, reg_channel = reg_config.split(':')
                reg_channel = int(reg_channel)
                layers, c_in = middle(input_channels)
                layers.append(nn.Conv2d(c_in, num_anchors_per_location * reg_channel, kernel_size=3, stride=1, padding=1, bias=True))
                code_size_cnt += reg_channel
                self.conv_box['conv_%s' % reg_name] = nn.Sequential(*layers)
                self.conv_box_names.append('conv_%s' % reg_name)
            for m in self.conv_box.modules():
                if isinstance(m, nn.Conv2d):
                    nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                    if m.bias is not None:
                        nn.init.constant_(m.bias, 0)
            assert code_size_cnt == code_size, 'Code size does not match: %d:%d' % (code_size_cnt, code_size)
        else:
            self.conv_cls = nn.Conv2d(input_channels, num_anchors_per_location * num_class, kernel_size=1)
            self.conv_box = nn.Conv2d(input_channels, num_anchors_per_location * code_size, kernel_size=1)
        if field(model_cfg, 'USE_DIRECTION_CLASSIFIER', None) is not None:
            self.conv_dir_cls = nn.Conv2d(input_channels, num_anchors_per_location * model_cfg['NUM_DIR_BINS'], kernel_size=1)
        else:
            self.conv_dir_cls = None
        self.use_multihead = field(model_cfg, 'USE_MULTIHEAD', False)
        self.init_weights()

    def init_weights(self):
        pi = 0.01
        last = self.conv_cls if isinstance(self.conv_cls, nn.Conv2d) else self.conv_cls[-1]
        nn.init.constant_(last.bias, -np.log((1 - pi) / pi))

    def _rows(self, x, columns):
        """(B, A * columns, H, W) -> (B, A * H * W, columns), the rows in the order of the class-major table."""
        B, _, H, W = x.shape
        return x.view(B, self.num_anchors_per_location, columns, H, W).permute(0, 1, 3, 4, 2).contiguous().view(B, -1, columns)

    def forward(self, spatial_features_2d):
        x = super().forward({'spatial_features': spatial_features_2d})['spatial_features_2d']
        cls_preds = self.conv_cls(x)
        if self.separate_reg_config is None:
            box_preds = self.conv_box(x)
        else:
            box_preds = torch.cat([self.conv_box[name](x) for name in self.conv_box_names], dim=1)
        dir_cls_preds = None
        if self.conv_dir_cls is not None:
            dir_cls_preds = self._rows(self.conv_dir_cls(x), self.model_cfg['NUM_DIR_BINS'])
        return {'cls_preds': self._rows(cls_preds, self.num_class), 'box_preds': self._rows(box_preds, self.code_size),
                'dir_cls_preds': dir_cls_preds}


class AnchorHeadMulti(AnchorHeadTemplate):
    MULTIHEAD = True

    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range,
                 predict_boxes_when_training=True, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class, class_names=class_names, grid_size=grid_size,
                         point_cloud_range=point_cloud_range, predict_boxes_when_training=predict_boxes_when_training)
        self.separate_multihead = field(model_cfg, 'SEPARATE_MULTIHEAD', False)
        if field(model_cfg, 'USE_DIRECTION_CLASSIFIER', None) is not None and not 1 <= model_cfg['NUM_DIR_BINS'] <= MAX_BINS:
            raise ValueError("NUM_DIR_BINS must lie in 1..%d" % MAX_BINS)
        if field(model_cfg, 'SHARED_CONV_NUM_FILTER', None) is not None:
            shared = model_cfg['SHARED_CONV_NUM_FILTER']
            self.shared_conv = nn.Sequential(nn.Conv2d(input_channels, shared, 3, stride=1, padding=1, bias=False),
                                             nn.BatchNorm2d(shared, eps=1e-3, momentum=0.01), nn.ReLU())
        else:
            self.shared_conv = None
            shared = input_channels
        self.rpn_heads = None
        self.make_multihead(shared)

    def get_target_assigner(self, anchor_target_cfg):
        if anchor_target_cfg['NAME'] != 'AxisAlignedTargetAssigner':
            raise NotImplementedError("TARGET_ASSIGNER_CONFIG.NAME: %s" % anchor_target_cfg['NAME'])
        return ClassMajorTargetAssigner(model_cfg=self.model_cfg, class_names=self.class_names, box_coder=self.box_coder,
                                        match_height=anchor_target_cfg['MATCH_HEIGHT'])

    def make_multihead(self, input_channels):
        rpn_head_cfgs = self.model_cfg['RPN_HEAD_CFGS']
        class_names = [name for cfg in rpn_head_cfgs for name in cfg['HEAD_CLS_NAME']]
        anchor_classes = [c['class_name'] for c in self.model_cfg['ANCHOR_GENERATOR_CONFIG']]
        if class_names != anchor_classes:
            raise ValueError("RPN_HEAD_CFGS lists the classes %s, ANCHOR_GENERATOR_CONFIG %s: the rows of the heads follow the "
                             "anchors only in the same order" % (class_names, anchor_classes))
        if not 1 <= len(rpn_head_cfgs) <= MAX_CLASSES:
            raise ValueError("1..%d heads, got %d" % (MAX_CLASSES, len(rpn_head_cfgs)))
        _, class_rows = class_major_table(self.anchors)
        rpn_heads, self.head_rows = [], []
        for rpn_head_cfg in rpn_head_cfgs:
            owned = [class_names.index(name) for name in rpn_head_cfg['HEAD_CLS_NAME']]
            num_anchors_per_location = sum(self.num_anchors_per_location[i] for i in owned)
            head_label_indices = torch.from_numpy(np.array([self.class_names.index(name) + 1
                                                            for name in rpn_head_cfg['HEAD_CLS_NAME']]))
            rpn_heads.append(SingleHead(
                self.model_cfg, input_channels, len(rpn_head_cfg['HEAD_CLS_NAME']) if self.separate_multihead else self.num_class,
                num_anchors_per_location, self.box_coder.code_size, rpn_head_cfg, head_label_indices=head_label_indices,
                separate_reg_config=field(self.model_cfg, 'SEPARATE_REG_CONFIG', None)))
            self.head_rows.append(sum(class_rows[i] for i in owned))
        self.rpn_heads = nn.ModuleList(rpn_heads)

    def forward(self, data_dict):
        spatial_features_2d = data_dict['spatial_features_2d']
        if self.shared_conv is not None:
            spatial_features_2d = self.shared_conv(spatial_features_2d)
        ret_dicts = [rpn_head(spatial_features_2d) for rpn_head in self.rpn_heads]
        gather = lambda key: ([r[key] for r in ret_dicts] if self.separate_multihead
                              else torch.cat([r[key] for r in ret_dicts], dim=1))
        ret = {'cls_preds': gather('cls_preds'), 'box_preds': gather('box_preds')}
        if field(self.model_cfg, 'USE_DIRECTION_CLASSIFIER', False):
            ret['dir_cls_preds'] = gather('dir_cls_preds')
        self.forward_ret_dict.update(ret)
        if self.training:
            self.forward_ret_dict.update(self.assign_targets(gt_boxes=data_dict['gt_boxes']))
        if not self.training or self.predict_boxes_when_training:
            batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(
                batch_size=data_dict['batch_size'], cls_preds=ret['cls_preds'], box_preds=ret['box_preds'],
                dir_cls_preds=ret.get('dir_cls_preds', None))
            if isinstance(batch_cls_preds, list):
                data_dict['multihead_label_mapping'] = [head.head_label_indices for head in self.rpn_heads]
            data_dict['batch_cls_preds'] = batch_cls_preds
            data_dict['batch_box_preds'] = batch_box_preds
            data_dict['cls_preds_normalized'] = False
        return data_dict

    def generate_predicted_boxes(self, batch_size, cls_preds, box_preds, dir_cls_preds=None):
        """cls_preds, box_preds, dir_cls_preds: (B, N, C) tensors, or lists of per-head (B, N_h, C_h) tensors ->
        batch_cls_preds (the list as it is, or (B, N, num_class)) and batch_box_preds (B, N, 7).  One launch."""
        join = lambda x: torch.cat(x, dim=1) if isinstance(x, list) else x
        table = self.anchor_table(join(box_preds).device)
        batch_cls_preds = cls_preds if isinstance(cls_preds, list) else cls_preds.view(batch_size, table.shape[0], -1).float()
        if dir_cls_preds is not None:
            boxes = anchor_decode(join(box_preds), join(dir_cls_preds), table, self.model_cfg['DIR_OFFSET'],
                                  self.model_cfg['DIR_LIMIT_OFFSET'])
        else:
            boxes = anchor_decode(join(box_preds), None, table)
        return batch_cls_preds, boxes

    def get_loss(self):
        """(rpn_loss, tb_dict) from forward_ret_dict: get_cls_layer_loss and get_box_reg_layer_loss of all heads in one pass.
        tb_dict holds 0-dim device tensors under the reference's keys."""
        ret = self.forward_ret_dict
        weights = self.model_cfg['LOSS_CONFIG']['LOSS_WEIGHTS']
        as_list = lambda x: x if isinstance(x, list) else [x]
        cls_preds = as_list(ret['cls_preds'])
        dir_preds = ret.get('dir_cls_preds', None)
        if self.separate_multihead:
            cols = [head.num_class for head in self.rpn_heads]
            bases = [sum(cols[:h]) for h in range(len(cols))]
        else:
            cols, bases = [self.num_class], [0]
        labels = ret['box_cls_labels']
        loss, out = anchor_multi_loss(
            cls_preds, as_list(ret['box_preds']), None if dir_preds is None else as_list(dir_preds), cols, bases, labels,
            ret['box_reg_targets'], ret['num_pos'], self.anchor_table(labels.device), self.num_class, weights['code_weights'],
            weights['cls_weight'], weights['loc_weight'], weights['dir_weight'] if dir_preds is not None else 0.0,
            self.model_cfg['DIR_OFFSET'] if dir_preds is not None else 0.0, field(weights, 'pos_cls_weight', 1.0),
            field(weights, 'neg_cls_weight', 1.0))
        tb_dict = {'rpn_loss_cls': out[0], 'rpn_loss_loc': out[1]}
        if dir_preds is not None:
            tb_dict['rpn_loss_dir'] = out[2]
        tb_dict['rpn_loss'] = out[3]
        return loss, tb_dict
