"""The anchor heads of the nuScenes yamls (nuscenes_models/cbgs_pp_multihead.yaml, cbgs_second_multihead.yaml): ResidualCoder
with encode_angle_by_sincos and / or code_size 9 (two velocity columns behind the heading), REG_LOSS_TYPE WeightedL1Loss.  The
classes of anchor_head.py and anchor_head_multi.py keep their 7-column contract and refuse these; the ones here take both,
under the same reference names, constructor signatures and state-dict keys, through the `_coded` entries of csrc/anchor_head.hip
(the same kernels, instantiated for the row width, the heading code and the regression term).

With extra = code_size - 7 custom columns and sincos = encode_angle_by_sincos a code row holds code = 6 + (2 if sincos else 1) +
extra columns; gt_boxes is (B, M, 8 + extra), the 1-based label last; decoded boxes are (B, N, 7 + extra).  The anchor table
stays (N, 7): the reference pads its anchors with zero columns (anchor_head_template.py:46-48), so a custom target is the gt's own
value -- a NaN velocity stays NaN in the targets and contributes 0 to the loss and its gradient -- and a decoded custom column
is the code's own.

Refused, NotImplementedError: what the parents refuse (POS_FRACTION >= 0, NORM_BY_NUM_EXAMPLES, MATCH_HEIGHT, ATSS, several
bottom heights, USE_MULTIHEAD: False on the multihead and True on the single head), a code_size outside 7..9, and
encode_angle_by_sincos with USE_DIRECTION_CLASSIFIER (the reference would take the sine difference of the cosine column and
add direction bins to an atan2; no yaml asks for it).  A gt_boxes whose column count disagrees with the coder: ValueError."""
import ctypes

import torch

from . import loss_utils
from .anchor_head import (MAX_BINS, MAX_CLASSES, AnchorHeadSingle, AxisAlignedTargetAssigner, _AnchorLoss)
from .anchor_head_multi import AnchorHeadMulti, ClassMajorTargetAssigner, _AnchorMultiLoss
from .config import field
from .pointnet2_batch_cuda import F32, I32, _call, _chk

REG_LOSS = {'WeightedSmoothL1Loss': 0, 'WeightedL1Loss': 1}      # include/pda_train.h PDA_REG_SMOOTH_L1, PDA_REG_L1


def code_layout(box_coder):
    """(code, sincos, extra) of a ResidualCoder: the columns of a code row, the heading flag and the custom columns."""
    sincos = int(bool(getattr(box_coder, 'encode_angle_by_sincos', False)))
    extra = box_coder.code_size - sincos - 7
    if not 0 <= extra <= 2:
        raise NotImplementedError("ResidualCoder code_size %d: 7 + at most two custom columns" % (box_coder.code_size - sincos))
    return 7 + sincos + extra, sincos, extra


class _CodedAssign(object):
    """assign_targets of both table layouts through the coded entries."""
    CODED = True

    def assign_targets(self, all_anchors, gt_boxes_with_classes):
        """gt_boxes (B, M, 8 + extra) -> box_cls_labels (B, N) int32, box_reg_targets (B, N, code), reg_weights (B, N) and
        num_pos (B) int32.  Two launches; no host read; gt_boxes is not written."""
        code, sincos, extra = code_layout(self.box_coder)
        gt = gt_boxes_with_classes
        if not isinstance(gt, torch.Tensor) or gt.dim() != 3 or gt.shape[-1] != 8 + extra:
            raise ValueError("gt_boxes must be a (B, M, %d) tensor for a ResidualCoder of %d box columns, got %s"
                             % (8 + extra, 7 + extra, tuple(getattr(gt, 'shape', ()))))
        _chk(gt, "gt_boxes", F32)
        B, M = gt.shape[0], gt.shape[1]
        table, counts = self.table(all_anchors, gt.device)
        N, dev = table.shape[0], gt.device
        labels = torch.empty((B, N), dtype=I32, device=dev)
        targets = torch.empty((B, N, code), dtype=F32, device=dev)
        weights = torch.empty((B, N), dtype=F32, device=dev)
        num_pos = torch.empty((B,), dtype=I32, device=dev)
        col_max = torch.empty((B, max(M, 1)), dtype=I32, device=dev)
        if B and N:
            _call(self.ENTRY, gt, gt.data_ptr(), 8 + extra, sincos, B, M, table.data_ptr(), N, len(self.anchor_class_names),
                  self._label_c, self._matched_c, self._unmatched_c, counts, col_max.data_ptr(), labels.data_ptr(),
                  targets.data_ptr(), weights.data_ptr(), num_pos.data_ptr())
        return {'box_cls_labels': labels, 'box_reg_targets': targets, 'reg_weights': weights, 'num_pos': num_pos}


class CodedAxisAlignedTargetAssigner(_CodedAssign, AxisAlignedTargetAssigner):
    ENTRY = "pda_anchor_assign_targets_coded"


class CodedClassMajorTargetAssigner(_CodedAssign, ClassMajorTargetAssigner):
    ENTRY = "pda_anchor_multi_assign_targets_coded"


def _coded_host(code, sincos, reg_loss, code_weights, has_dir):
    if isinstance(reg_loss, str):
        if reg_loss not in REG_LOSS:
            raise NotImplementedError("REG_LOSS_TYPE %r (%s)" % (reg_loss, ", ".join(REG_LOSS)))
        reg_loss = REG_LOSS[reg_loss]
    if sincos not in (0, 1) or not 7 + sincos <= code <= 9 + sincos:
        raise ValueError("code=%d, sincos=%r: a code holds 6 + (2 if sincos else 1) + 0..2 columns" % (code, sincos))
    if sincos and has_dir:
        raise NotImplementedError("encode_angle_by_sincos with a direction classifier")
    if len(code_weights) != code:
        raise ValueError("%d code weights for a code of %d columns" % (len(code_weights), code))
    return (ctypes.c_float * code)(*[float(w) for w in code_weights]), (int(code), int(sincos), int(reg_loss))


def anchor_loss_coded(cls_preds, box_preds, dir_cls_preds, box_cls_labels, box_reg_targets, num_pos, table, num_class, code_weights,
                      cls_weight, loc_weight, dir_weight=0.0, dir_offset=0.0, sincos=0, reg_loss='WeightedSmoothL1Loss'):
    """anchor_head.anchor_loss for code rows of box_reg_targets.shape[2] columns: box_preds (B, N, code), targets (B, N, code),
    code_weights (code); reg_loss a REG_LOSS_TYPE.  Without sincos the sine difference is taken on column 6, as there."""
    B, N = box_cls_labels.shape
    code = box_reg_targets.shape[-1]
    preds = [cls_preds.reshape(B, N, -1).contiguous(), box_preds.reshape(B, N, -1).contiguous(),
             None if dir_cls_preds is None else dir_cls_preds.reshape(B, N, -1).contiguous()]
    code_w, coded = _coded_host(code, sincos, reg_loss, code_weights, preds[2] is not None)
    for name, t in zip(("cls_preds", "box_preds", "dir_cls_preds"), preds):
        if t is not None:
            _chk(t, name, F32)
    _chk(box_cls_labels, "box_cls_labels", I32), _chk(box_reg_targets, "box_reg_targets", F32), _chk(num_pos, "num_pos", I32)
    _chk(table, "anchors", F32)
    if preds[0].shape[2] != num_class or not 1 <= num_class <= MAX_CLASSES:
        raise ValueError("cls_preds %s do not hold %d classes (at most %d)" % (tuple(cls_preds.shape), num_class, MAX_CLASSES))
    if preds[1].shape[2] != code or tuple(box_reg_targets.shape) != (B, N, code) or table.shape != (N, 7) or num_pos.numel() != B:
        raise ValueError("box_preds, box_reg_targets, anchors and num_pos must be (B, N, %d), (B, N, %d), (N, 7) and (B)" % (code, code))
    bins = 0 if preds[2] is None else preds[2].shape[2]
    if bins > MAX_BINS:
        raise ValueError("at most %d direction bins, got %d" % (MAX_BINS, bins))
    if B * N == 0:
        raise ValueError("an empty batch has no loss")
    host = (code_w, float(cls_weight), float(loc_weight), float(dir_weight), float(dir_offset), int(num_class), int(bins)) + coded
    return _AnchorLoss.apply(preds[0], preds[1], preds[2], box_cls_labels, box_reg_targets, num_pos, table, host)


def anchor_multi_loss_coded(cls_preds, box_preds, dir_cls_preds, head_cols, head_col_base, box_cls_labels, box_reg_targets, num_pos,
                            table, num_class, code_weights, cls_weight, loc_weight, dir_weight=0.0, dir_offset=0.0,
                            pos_cls_weight=1.0, neg_cls_weight=1.0, sincos=0, reg_loss='WeightedSmoothL1Loss'):
    """anchor_head_multi.anchor_multi_loss for code rows of box_reg_targets.shape[2] columns: box_preds[h] (B, N_h, code),
    targets (B, N, code), code_weights (code); reg_loss a REG_LOSS_TYPE.  Returns (rpn_loss, out) as there."""
    B, N = box_cls_labels.shape
    H = len(cls_preds)
    code = box_reg_targets.shape[-1]
    if not 1 <= H <= MAX_CLASSES or len(box_preds) != H or len(head_cols) != H or len(head_col_base) != H:
        raise ValueError("1..%d heads with one cls_preds, box_preds, column count and column base each" % MAX_CLASSES)
    if dir_cls_preds is not None and len(dir_cls_preds) != H:
        raise ValueError("dir_cls_preds must hold one tensor per head")
    code_w, coded = _coded_host(code, sincos, reg_loss, code_weights, dir_cls_preds is not None)
    if B * N == 0:
        raise ValueError("an empty batch has no loss")
    _chk(box_cls_labels, "box_cls_labels", I32), _chk(box_reg_targets, "box_reg_targets", F32), _chk(num_pos, "num_pos", I32)
    _chk(table, "anchors", F32)
    if tuple(box_reg_targets.shape) != (B, N, code) or tuple(table.shape) != (N, 7) or num_pos.numel() != B:
        raise ValueError("box_reg_targets, anchors and num_pos must be (B, N, %d), (N, 7) and (B)" % code)
    cls, box, dirs, rows = [], [], [], []
    for h in range(H):
        b = box_preds[h].reshape(B, -1, code).contiguous()
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
    host = (rows, [int(v) for v in head_cols], [int(v) for v in head_col_base], int(num_class), int(bins), code_w,
            (float(cls_weight), float(loc_weight), float(dir_weight) if dirs else 0.0, float(dir_offset) if dirs else 0.0,
             float(pos_cls_weight), float(neg_cls_weight))) + coded
    return _AnchorMultiLoss.apply(host, box_cls_labels, box_reg_targets, num_pos, table, *cls, *box, *dirs)


@torch.no_grad()
def anchor_decode_coded(box_preds, dir_cls_preds, table, dir_offset=0.0, dir_limit_offset=0.0, sincos=0):
    """box_preds (B, N, code), dir_cls_preds (B, N, bins) or None (always None with sincos), table (N, 7) -> batch_box_preds
    (B, N, code - sincos): the box, its heading from the scalar residual or the cos / sin pair, the custom columns.  One launch."""
    B, N = box_preds.shape[0], table.shape[0]
    box = box_preds.detach().reshape(B, N, -1).contiguous()
    _chk(box, "box_preds", F32), _chk(table, "anchors", F32)
    code = box.shape[2]
    _coded_host(code, sincos, 0, [1.0] * code, dir_cls_preds is not None)
    dirs = None
    if dir_cls_preds is not None:
        dirs = dir_cls_preds.detach().reshape(B, N, -1).contiguous()
        _chk(dirs, "dir_cls_preds", F32)
        if dirs.shape[2] > MAX_BINS:
            raise ValueError("at most %d direction bins, got %d" % (MAX_BINS, dirs.shape[2]))
    out = torch.empty((B, N, code - sincos), dtype=F32, device=box.device)
    if B * N:
        _call("pda_anchor_decode_coded", box, code, int(sincos), box.data_ptr(), None if dirs is None else dirs.data_ptr(),
              table.data_ptr(), B, N, 0 if dirs is None else dirs.shape[2], float(dir_offset), float(dir_limit_offset), out.data_ptr())
    return out


class _CodedHead(object):
    """What AnchorHeadSingleCoded and AnchorHeadMultiCoded change of AnchorHeadTemplate: the coder's contract, the assigner,
    the regression term, and the coded decode."""
    CODED = True
    ASSIGNER = None

    def get_target_assigner(self, anchor_target_cfg):
        code_layout(self.box_coder)
        if self.box_coder.encode_angle_by_sincos and field(self.model_cfg, 'USE_DIRECTION_CLASSIFIER', None) is not None:
            raise NotImplementedError("encode_angle_by_sincos with USE_DIRECTION_CLASSIFIER")
        if anchor_target_cfg['NAME'] != 'AxisAlignedTargetAssigner':
            raise NotImplementedError("TARGET_ASSIGNER_CONFIG.NAME: %s" % anchor_target_cfg['NAME'])
        return self.ASSIGNER(model_cfg=self.model_cfg, class_names=self.class_names, box_coder=self.box_coder,
                             match_height=anchor_target_cfg['MATCH_HEIGHT'])

    def build_losses(self, losses_cfg):
        self.reg_loss_type = field(losses_cfg, 'REG_LOSS_TYPE', None) or 'WeightedSmoothL1Loss'
        if self.reg_loss_type not in REG_LOSS:
            raise NotImplementedError("REG_LOSS_TYPE %r" % (self.reg_loss_type,))
        code, _, _ = code_layout(self.box_coder)
        code_weights = losses_cfg['LOSS_WEIGHTS']['code_weights']
        if len(code_weights) != code:
            raise ValueError("%d code_weights for a code of %d columns" % (len(code_weights), code))
        # the reference's modules, for users of its names; get_loss takes the fused path
        self.add_module('cls_loss_func', loss_utils.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0))
        self.add_module('reg_loss_func', getattr(loss_utils, self.reg_loss_type)(code_weights=code_weights))
        self.add_module('dir_loss_func', loss_utils.WeightedCrossEntropyLoss())

    def decode(self, box_preds, dir_cls_preds, table):
        sincos = code_layout(self.box_coder)[1]
        if dir_cls_preds is not None:
            return anchor_decode_coded(box_preds, dir_cls_preds, table, self.model_cfg['DIR_OFFSET'], self.model_cfg['DIR_LIMIT_OFFSET'],
                                       sincos=sincos)
        return anchor_decode_coded(box_preds, None, table, sincos=sincos)

    def loss_kwargs(self, dir_preds):
        weights = self.model_cfg['LOSS_CONFIG']['LOSS_WEIGHTS']
        return dict(num_class=self.num_class, code_weights=weights['code_weights'], cls_weight=weights['cls_weight'],
                    loc_weight=weights['loc_weight'], dir_weight=weights['dir_weight'] if dir_preds is not None else 0.0,
                    dir_offset=self.model_cfg['DIR_OFFSET'] if dir_preds is not None else 0.0,
                    sincos=code_layout(self.box_coder)[1], reg_loss=self.reg_loss_type)

    @staticmethod
    def tb_dict(out, has_dir):
        tb = {'rpn_loss_cls': out[0], 'rpn_loss_loc': out[1]}
        if has_dir:
            tb['rpn_loss_dir'] = out[2]
        tb['rpn_loss'] = out[3]
        return tb


class AnchorHeadSingleCoded(_CodedHead, AnchorHeadSingle):
    ASSIGNER = CodedAxisAlignedTargetAssigner

    def get_loss(self):
        ret = self.forward_ret_dict
        dir_preds = ret.get('dir_cls_preds', None)
        labels = ret['box_cls_labels']
        loss, out = anchor_loss_coded(ret['cls_preds'], ret['box_preds'], dir_preds, labels, ret['box_reg_targets'], ret['num_pos'],
                                      self.anchor_table(labels.device), **self.loss_kwargs(dir_preds))
        return loss, self.tb_dict(out, dir_preds is not None)

    def generate_predicted_boxes(self, batch_size, cls_preds, box_preds, dir_cls_preds=None):
        table = self.anchor_table(box_preds.device)
        return cls_preds.view(batch_size, table.shape[0], -1).float(), self.decode(box_preds, dir_cls_preds, table)


class AnchorHeadMultiCoded(_CodedHead, AnchorHeadMulti):
    ASSIGNER = CodedClassMajorTargetAssigner

    def get_loss(self):
        """(rpn_loss, tb_dict) from forward_ret_dict, all heads in one pass; tb_dict holds 0-dim device tensors."""
        ret = self.forward_ret_dict
        weights = self.model_cfg['LOSS_CONFIG']['LOSS_WEIGHTS']
        as_list = lambda x: x if isinstance(x, list) else [x]
        dir_preds = ret.get('dir_cls_preds', None)
        if self.separate_multihead:
            cols = [head.num_class for head in self.rpn_heads]
            bases = [sum(cols[:h]) for h in range(len(cols))]
        else:
            cols, bases = [self.num_class], [0]
        labels = ret['box_cls_labels']
        loss, out = anchor_multi_loss_coded(
            as_list(ret['cls_preds']), as_list(ret['box_preds']), None if dir_preds is None else as_list(dir_preds), cols, bases,
            labels, ret['box_reg_targets'], ret['num_pos'], self.anchor_table(labels.device),
            pos_cls_weight=field(weights, 'pos_cls_weight', 1.0), neg_cls_weight=field(weights, 'neg_cls_weight', 1.0),
            **self.loss_kwargs(dir_preds))
        return loss, self.tb_dict(out, dir_preds is not None)

    def generate_predicted_boxes(self, batch_size, cls_preds, box_preds, dir_cls_preds=None):
        """As AnchorHeadMulti's, batch_box_preds (B, N, 7 + extra).  One launch."""
        join = lambda x: torch.cat(x, dim=1) if isinstance(x, list) else x
        table = self.anchor_table(join(box_preds).device)
        batch_cls_preds = cls_preds if isinstance(cls_preds, list) else cls_preds.view(batch_size, table.shape[0], -1).float()
        return batch_cls_preds, self.decode(join(box_preds), None if dir_cls_preds is None else join(dir_cls_preds), table)
