"""Post-processing of the detector (pcdet/models/detectors/detector3d_template.py:179-290 with
MULTI_CLASSES_NMS False -> model_utils/model_nms_utils.py:6-27 class_agnostic_nms), for all scenes
of a batch at once and without host synchronisation until the final compaction.

Reference, per scene: sigmoid -> max over classes -> `scores >= SCORE_THRESH` compaction -> topk
(NMS_PRE_MAXSIZE) -> nms_gpu (sort, mask kernel, device->host copy, host scan) -> first
NMS_POST_MAXSIZE -> index back.  Here: one masked sort for the batch, one gather, `nms_batched`
(csrc/iou3d_nms.hip) with per-scene valid counts, one gather.

Recall (detector3d_template.py:271-276, 288-329, with RECALL_MODE 'normal' and a batch that carries gt_boxes): the
reference trims each scene's GT, runs boxes_iou3d_gpu and reads one count per threshold back to the host.  Here
`recall_record` (csrc/recall.hip) adds the whole batch's counts to device counters in one launch; post_processing keeps
them under padded['recall'], `to_pred_and_recall_dicts` reads them with the counts it reads anyway, and `RecallRecorder`
sums them over an eval loop."""
import ctypes

import torch

from . import iou3d_nms_utils
from .pointnet2_batch_cuda import F32, I32, _call, _chk

MAX_RECALL_THRESH = 16


def class_agnostic_nms_batched(box_scores, box_preds, nms_config, score_thresh=None, valid=None):
    """box_scores (B, N), box_preds (B, N, 7+C).  Returns selected (B, K) int64 indices into N (-1 padded),
    their scores (B, K) (0 padded) and num_selected (B) int32, K = min(N, NMS_POST_MAXSIZE).  valid (B, N) bool, optional:
    rows that take part at all (the padded rows of a caller whose scenes hold different numbers of boxes)."""
    B, N = box_scores.shape
    if nms_config["NMS_TYPE"] not in ("nms_gpu", "nms_normal_gpu"):
        raise NotImplementedError(nms_config["NMS_TYPE"])
    ok = box_scores >= score_thresh if score_thresh is not None else torch.ones_like(box_scores, dtype=torch.bool)
    valid = ok if valid is None else ok & valid
    masked = torch.where(valid, box_scores, torch.full_like(box_scores, float("-inf")))
    sorted_scores, order = masked.sort(dim=1, descending=True)
    pre = int(nms_config["NMS_PRE_MAXSIZE"])
    num_valid = valid.sum(dim=1).clamp(max=pre).to(torch.int32)
    K = min(N, int(nms_config["NMS_POST_MAXSIZE"]))
    # the NMS looks at the first num_valid <= NMS_PRE_MAXSIZE rows of the ranking only: the rest is not handed to it (the anchors
    # of a full KITTI grid, 211 200 a scene, are more than one call takes)
    width = min(N, max(pre, K))
    boxes = torch.gather(box_preds[..., 0:7], 1, order[:, :width].unsqueeze(-1).expand(B, width, 7)).contiguous()
    keep, num_keep = iou3d_nms_utils.nms_batched(boxes, nms_config["NMS_THRESH"], num_valid=num_valid,
                                                 normal=nms_config["NMS_TYPE"] == "nms_normal_gpu")
    keep = keep[:, :K]
    ok = keep >= 0
    safe = keep.clamp(min=0)
    selected = torch.where(ok, torch.gather(order, 1, safe), torch.full_like(keep, -1))
    scores = torch.where(ok, torch.gather(sorted_scores, 1, safe), torch.zeros_like(sorted_scores[:, :K]))
    return selected, scores, num_keep.clamp(max=K)


def _selected_rows(nms, box_preds, **rows):
    """The padded tensors of class_agnostic_nms_batched's result `nms`: box_preds (B, N, 7+C) and each (B, N) tensor of `rows`
    at selected (B, K), zero where selected is -1.  The boxes are multiplied by the mask, the others go through torch.where;
    the two differ for non-finite rows.  A `pred_scores` among the rows takes the place of the scores the NMS ranked by."""
    selected, sel_scores, num = nms
    ok = selected >= 0
    safe = selected.clamp(min=0)
    padded = {'pred_boxes': torch.gather(box_preds, 1, safe.unsqueeze(-1).expand(-1, -1, box_preds.shape[-1])) * ok.unsqueeze(-1),
              'pred_scores': sel_scores, 'num_pred': num}
    for k, x in rows.items():
        padded[k] = torch.where(ok, torch.gather(x, 1, safe), torch.zeros_like(x[:, :safe.shape[1]]))
    return padded


def _with_recall(padded, batch_dict, post_process_cfg, rois=None):
    """padded with 'recall', (1 + n) int64 [gt, rcnn_<t>...] of this batch on the device, when RECALL_MODE is 'normal' (the
    default) and the batch carries gt_boxes: counted on padded's boxes, or on all rows of rois (B, N, 7) when given."""
    if post_process_cfg.get('RECALL_MODE', 'normal') == 'normal' and 'gt_boxes' in batch_dict:
        boxes, num = padded['pred_boxes'], padded['num_pred']
        if rois is not None:
            boxes, num = rois.contiguous(), torch.full_like(num, rois.shape[1])
            padded['recall_on_rois'] = True
        padded['recall'] = recall_record(boxes, num, batch_dict['gt_boxes'], post_process_cfg['RECALL_THRESH_LIST'])
    return padded


def post_processing(batch_dict, post_process_cfg, num_class):
    """detector3d_template.py:179-290 for point heads (`batch_index` layout, equal points per scene); with
    NMS_CONFIG.MULTI_CLASSES_NMS and a list batch_cls_preds (a separate multihead) multi_classes_nms_batched.
    Returns padded device tensors: pred_boxes (B, K, 7+C), pred_scores (B, K), pred_labels (B, K) int64
    (0 = padding) and num_pred (B) int32; with RECALL_MODE 'normal' (the default) and gt_boxes in batch_dict also
    recall (1 + len(RECALL_THRESH_LIST)) int64 [gt, rcnn_<t>...], this batch's recall counts."""
    if post_process_cfg["NMS_CONFIG"]["MULTI_CLASSES_NMS"]:
        if not isinstance(batch_dict['batch_cls_preds'], list):
            raise NotImplementedError("MULTI_CLASSES_NMS with one batch_cls_preds tensor (the reference's arange(1, num_class) "
                                      "label mapping fails its own assertion there); a separate multihead passes a list")
        return _post_processing_multi_classes(batch_dict, post_process_cfg)
    B = batch_dict['batch_size']
    box_preds = batch_dict['batch_box_preds'].view(B, -1, batch_dict['batch_box_preds'].shape[-1])
    cls_preds = batch_dict['batch_cls_preds'].view(B, box_preds.shape[1], -1)
    assert cls_preds.shape[-1] in (1, num_class)
    src_cls_preds = cls_preds
    if not batch_dict['cls_preds_normalized']:
        cls_preds = torch.sigmoid(cls_preds)
    scores, labels = torch.max(cls_preds, dim=-1)
    valid = None
    if batch_dict.get('has_class_labels', False):
        # a two-stage head scores class-agnostically: the labels are the first stage's (detector3d_template.py:238-240)
        labels = batch_dict['roi_labels' if 'roi_labels' in batch_dict else 'batch_pred_labels'].view(B, -1)
        if 'roi_labels' in batch_dict:
            # CenterHead pads its RoIs with zero boxes of label 0 (proposal_layer's padding carries label 1): such a row is no
            # proposal and does not become a prediction, whatever the second stage scores it (the reference lets it through)
            valid = labels > 0
    else:
        labels = labels + 1
    nms = class_agnostic_nms_batched(scores, box_preds, post_process_cfg["NMS_CONFIG"], score_thresh=post_process_cfg["SCORE_THRESH"],
                                     valid=valid)
    rows = {'pred_labels': labels}
    if post_process_cfg.get("OUTPUT_RAW_SCORE", False):
        rows['pred_scores'] = torch.max(src_cls_preds, dim=-1)[0]
    return _with_recall(_selected_rows(nms, box_preds, **rows), batch_dict, post_process_cfg)


def multi_classes_nms_batched(cls_preds, box_preds, label_mapping, nms_config, score_thresh=None, normalized=False):
    """model_nms_utils.multi_classes_nms under detector3d_template.post_processing's loop over heads, for all scenes at once.
    cls_preds: a list of per-head (B, N_h, C_h) logits (scores when `normalized`); box_preds (B, sum N_h, >= 7), head h owning
    the N_h rows behind those of the heads before it; label_mapping: per head the (C_h) 1-based labels of its columns.
    Every (scene, head, class column) is one NMS problem: its scores >= score_thresh, sorted, the first
    min(N_h, NMS_PRE_MAXSIZE) of them gathered -- only those rows, so a head may have more rows than pda_nms_bev takes --
    and all problems go through one pda_nms_bev and one pda_multi_nms_compact.  box_preds of 8 or 9 columns (velocities)
    keep their columns: pda_nms_bev reads a contiguous copy of columns 0..6, pda_multi_nms_compact_wide copies whole rows, and
    pred_boxes is (B, K, 7 + extra).  Returns pred_boxes (B, K, 7), pred_scores
    (B, K), pred_labels (B, K) int64 (0 = padding) and num_pred (B) int32, K = sum C_h * min(NMS_POST_MAXSIZE, max_h
    min(N_h, NMS_PRE_MAXSIZE)); a scene's rows run head after head, class column after class column, by descending score, as
    the reference concatenates them.  No host read.  Equal scores within a column are outside the parity claim: the
    reference leaves their order to topk, this to sort."""
    if nms_config["NMS_TYPE"] not in ("nms_gpu", "nms_normal_gpu"):
        raise NotImplementedError(nms_config["NMS_TYPE"])
    if len(cls_preds) != len(label_mapping) or not cls_preds:
        raise ValueError("one label mapping per head")
    B = box_preds.shape[0]
    pre, post = int(nms_config["NMS_PRE_MAXSIZE"]), int(nms_config["NMS_POST_MAXSIZE"])
    if sum(x.shape[1] for x in cls_preds) != box_preds.shape[1]:
        raise ValueError("the heads score %d rows, box_preds has %d" % (sum(x.shape[1] for x in cls_preds), box_preds.shape[1]))
    W = box_preds.shape[2]
    if not 7 <= W <= 9:
        raise NotImplementedError("box_preds with %d columns (7 + at most two custom columns)" % W)
    K = max(min(x.shape[1], pre) for x in cls_preds)
    boxes, scores, num_valid = [], [], []
    start = 0
    for x, mapping in zip(cls_preds, label_mapping):
        n, c = x.shape[1], x.shape[2]
        assert c == len(mapping)
        k = min(n, pre)
        s = (x if normalized else torch.sigmoid(x)).transpose(1, 2)                                  # (B, c, n)
        ok = s >= score_thresh if score_thresh is not None else torch.ones_like(s, dtype=torch.bool)
        sorted_scores, order = torch.where(ok, s, torch.full_like(s, float("-inf"))).sort(dim=2, descending=True)
        sorted_scores, order = sorted_scores[..., :k], order[..., :k]          # before the gather: k rows a problem, not n
        rows = box_preds[:, start:start + n].unsqueeze(1).expand(B, c, n, W)
        picked = torch.gather(rows, 2, order.unsqueeze(-1).expand(B, c, k, W))
        boxes.append(torch.nn.functional.pad(picked, (0, 0, 0, K - k)))
        scores.append(torch.nn.functional.pad(sorted_scores, (0, K - k)))
        num_valid.append(ok.sum(dim=2).clamp(max=k).to(torch.int32))
        start += n
    boxes = torch.cat(boxes, dim=1).to(F32).contiguous()                                             # (B, C, K, W)
    scores = torch.cat(scores, dim=1).to(F32).contiguous()
    num_valid = torch.cat(num_valid, dim=1).contiguous()
    C = boxes.shape[1]
    labels = torch.cat([m.reshape(-1) for m in label_mapping]).to(device=boxes.device, dtype=torch.int32).contiguous()
    bev = boxes if W == 7 else boxes[..., :7].contiguous()
    keep, num_keep = iou3d_nms_utils.nms_batched(bev.view(B * C, K, 7), nms_config["NMS_THRESH"], num_valid=num_valid.view(-1),
                                                 normal=nms_config["NMS_TYPE"] == "nms_normal_gpu")
    rows = C * min(post, K)
    dev = boxes.device
    pred_boxes = torch.empty((B, rows, W), dtype=F32, device=dev)
    pred_scores = torch.empty((B, rows), dtype=F32, device=dev)
    pred_labels = torch.empty((B, rows), dtype=torch.int64, device=dev)
    num_pred = torch.empty((B,), dtype=torch.int32, device=dev)
    if B:
        _call(*(("pda_multi_nms_compact", boxes) if W == 7 else ("pda_multi_nms_compact_wide", boxes, W)), _chk(boxes, "boxes", F32), _chk(scores, "scores", F32), _chk(keep, "keep", torch.int64),
              _chk(num_keep, "num_keep", I32), _chk(labels, "label_mapping", I32), B, C, K, post, pred_boxes.data_ptr(),
              pred_scores.data_ptr(), pred_labels.data_ptr(), num_pred.data_ptr())
    return pred_boxes, pred_scores, pred_labels, num_pred


def _post_processing_multi_classes(batch_dict, post_process_cfg):
    """post_processing with NMS_CONFIG.MULTI_CLASSES_NMS and a list batch_cls_preds (detector3d_template.py:225-250)."""
    B = batch_dict['batch_size']
    box_preds = batch_dict['batch_box_preds'].view(B, -1, batch_dict['batch_box_preds'].shape[-1])
    pred_boxes, pred_scores, pred_labels, num = multi_classes_nms_batched(
        batch_dict['batch_cls_preds'], box_preds, batch_dict['multihead_label_mapping'], post_process_cfg["NMS_CONFIG"],
        score_thresh=post_process_cfg["SCORE_THRESH"], normalized=batch_dict['cls_preds_normalized'])
    padded = {'pred_boxes': pred_boxes, 'pred_scores': pred_scores, 'pred_labels': pred_labels, 'num_pred': num}
    return _with_recall(padded, batch_dict, post_process_cfg)


PRED_KEYS = ('pred_boxes', 'pred_scores', 'pred_labels')
IOU_PRED_KEYS = PRED_KEYS + ('pred_cls_scores', 'pred_iou_scores')


def to_pred_dicts(padded):
    """The reference's return value: a list (one per scene) of {'pred_boxes','pred_scores','pred_labels'}
    with variable-length tensors.  One host synchronisation for the whole batch."""
    return _split(padded, padded['num_pred'].tolist())


def _split(padded, counts, keys=PRED_KEYS):
    return [{k: padded[k][s, :n] for k in keys} for s, n in enumerate(counts)]


def to_pred_and_recall_dicts(padded, thresh_list, keys=PRED_KEYS):
    """Detector3DTemplate.post_processing's return value (pred_dicts, recall_dict): the pred dicts hold `keys`; the recall dict
    holds 'gt' and 'roi_<t>' / 'rcnn_<t>' for every t of thresh_list (the RECALL_THRESH_LIST post_processing used) when padded
    carries the batch's recall counters, and is {} otherwise; roi_<t> equals rcnn_<t> when the recall was counted on the RoIs
    (SECONDHead's boxes ARE its RoIs).  The counters come back in the one host read that the counts need anyway."""
    B = padded['num_pred'].shape[0]
    has_recall = 'recall' in padded
    h = (torch.cat([padded['num_pred'].to(torch.int64), padded['recall']]) if has_recall else padded['num_pred']).tolist()
    preds = _split(padded, h[:B], keys)
    if not has_recall or B == 0:
        return preds, {}
    ret = recall_dict(h[B:], thresh_list)
    if padded.get('recall_on_rois', False):
        for t in thresh_list:
            ret['roi_%s' % str(t)] = ret['rcnn_%s' % str(t)]
    return preds, ret


def to_iou_pred_and_recall_dicts(padded, thresh_list):
    """SECONDNetIoU.post_processing's return value from post_processing_iou's tensors: the pred dicts hold IOU_PRED_KEYS."""
    return to_pred_and_recall_dicts(padded, thresh_list, IOU_PRED_KEYS)


IOU_SCORE_TYPES = ('iou', 'cls', 'weighted_iou_cls', 'num_pts_iou_cls', 'score_by_class')


def scores_by_npoints(cls_scores, iou_scores, num_points, cls_thresh=10, iou_thresh=100):
    """SECONDNetIoU.cal_scores_by_npoints (second_net_iou.py:37-57): the first-stage score up to cls_thresh points in the box,
    the IoU score from iou_thresh on, and between them alpha = (n - 10) / (iou_thresh - cls_thresh) -- with the literal 10,
    as the reference has it."""
    assert iou_thresh >= cls_thresh
    n = num_points.to(torch.float32)
    alpha = (n >= iou_thresh).to(torch.float32)
    if iou_thresh > cls_thresh:
        between = (n > cls_thresh) & (n < iou_thresh)
        alpha = torch.where(between, (n - 10) / (iou_thresh - cls_thresh), alpha)
    return (1 - alpha) * cls_scores + alpha * iou_scores


def nms_scores_by_class(iou_preds, cls_preds, label_preds, score_by_class, class_names):
    """SECONDNetIoU.set_nms_score_by_class (:59-73) for (B, N) tensors without its host read: the reference loops i over
    range(number of DISTINCT labels in the scene), so only classes i < that number receive a score and the others stay 0.
    The number is counted on the device from the sorted labels."""
    for name in class_names:
        if score_by_class[name] not in ('iou', 'cls'):
            raise NotImplementedError("SCORE_BY_CLASS[%r] = %r" % (name, score_by_class[name]))
    nms_scores = torch.zeros_like(iou_preds, dtype=torch.float32)
    if label_preds.shape[1] == 0:
        return nms_scores
    ordered = label_preds.sort(dim=1)[0]
    n_classes = 1 + (ordered[:, 1:] != ordered[:, :-1]).sum(dim=1, keepdim=True)               # (B, 1)
    for i, name in enumerate(class_names):
        mask = (label_preds == (i + 1)) & (n_classes > i)
        nms_scores = torch.where(mask, iou_preds if score_by_class[name] == 'iou' else cls_preds, nms_scores)
    return nms_scores


def post_processing_iou(batch_dict, post_process_cfg, num_class, class_names):
    """SECONDNetIoU.post_processing (second_net_iou.py:75-177) for all scenes of a batch at once: batch_cls_preds
    (B, N, 1 | num_class) is the IoU branch, roi_scores (B, N) the first stage's score, batch_box_preds (B, N, 7) the RoIs.
    Both scores go through a sigmoid unless cls_preds_normalized; NMS_CONFIG.SCORE_TYPE picks what the NMS ranks by
    ('iou', also when absent; 'cls'; 'weighted_iou_cls' with SCORE_WEIGHTS; 'num_pts_iou_cls' with SCORE_THRESH and the
    batch's `points`, counted by roiaware_pool3d_utils.points_in_boxes_count; 'score_by_class' with SCORE_BY_CLASS).
    Returns post_processing's padded tensors plus pred_cls_scores and pred_iou_scores (B, K) and nms_scores (B, N); recall,
    when the batch carries gt_boxes, is counted on the RoIs -- all N rows of a scene, as the reference does when
    batch_dict has 'rois' -- and padded['recall_on_rois'] says so.  No host read."""
    nms_cfg = post_process_cfg['NMS_CONFIG']
    if nms_cfg['MULTI_CLASSES_NMS']:
        raise NotImplementedError("MULTI_CLASSES_NMS")
    if post_process_cfg.get('OUTPUT_RAW_SCORE', False):
        raise NotImplementedError("OUTPUT_RAW_SCORE")
    B = batch_dict['batch_size']
    box_preds = batch_dict['batch_box_preds'].view(B, -1, batch_dict['batch_box_preds'].shape[-1])
    N = box_preds.shape[1]
    iou_preds = batch_dict['batch_cls_preds'].view(B, N, -1)
    cls_preds = batch_dict['roi_scores'].view(B, N)
    assert iou_preds.shape[-1] in (1, num_class)
    if not batch_dict['cls_preds_normalized']:
        iou_preds = torch.sigmoid(iou_preds)
        cls_preds = torch.sigmoid(cls_preds)
    iou_preds, label_preds = torch.max(iou_preds, dim=-1)
    label_preds = batch_dict['roi_labels'].view(B, N) if batch_dict.get('has_class_labels', False) else label_preds + 1

    score_type = nms_cfg.get('SCORE_TYPE', None)
    if nms_cfg.get('SCORE_BY_CLASS', None) and score_type == 'score_by_class':
        nms_scores = nms_scores_by_class(iou_preds, cls_preds, label_preds, nms_cfg['SCORE_BY_CLASS'], class_names)
    elif score_type == 'iou' or score_type is None:
        nms_scores = iou_preds
    elif score_type == 'cls':
        nms_scores = cls_preds
    elif score_type == 'weighted_iou_cls':
        nms_scores = nms_cfg['SCORE_WEIGHTS']['iou'] * iou_preds + nms_cfg['SCORE_WEIGHTS']['cls'] * cls_preds
    elif score_type == 'num_pts_iou_cls':
        from .roiaware_pool3d_utils import points_in_boxes_count
        counts = points_in_boxes_count(batch_dict['points'], box_preds[..., 0:7])
        nms_scores = scores_by_npoints(cls_preds, iou_preds, counts, nms_cfg['SCORE_THRESH']['cls'], nms_cfg['SCORE_THRESH']['iou'])
    else:
        raise NotImplementedError("NMS_CONFIG.SCORE_TYPE %r (%s)" % (score_type, ", ".join(IOU_SCORE_TYPES)))

    nms = class_agnostic_nms_batched(nms_scores, box_preds, nms_cfg, score_thresh=post_process_cfg["SCORE_THRESH"])
    padded = _selected_rows(nms, box_preds, pred_labels=label_preds, pred_cls_scores=cls_preds, pred_iou_scores=iou_preds)
    padded['nms_scores'] = nms_scores
    return _with_recall(padded, batch_dict, post_process_cfg, rois=box_preds if 'rois' in batch_dict else None)


def recall_dict(counts, thresh_list):
    """Host counters [gt, rcnn_<t>...] -> generate_recall_record's dict, in its key order (roi_* is 0: no rois)."""
    ret = {'gt': int(counts[0])}
    for i, t in enumerate(thresh_list):
        ret['roi_%s' % str(t)] = 0
        ret['rcnn_%s' % str(t)] = int(counts[1 + i])
    return ret


def _thresh_array(thresh_list):
    thresh_list = list(thresh_list)
    if len(thresh_list) > MAX_RECALL_THRESH:
        raise ValueError("at most %d recall thresholds, got %d" % (MAX_RECALL_THRESH, len(thresh_list)))
    return (ctypes.c_float * max(len(thresh_list), 1))(*[float(t) for t in thresh_list]), len(thresh_list)


def recall_record(pred_boxes, num_pred, gt_boxes, thresh_list, counters=None, max_iou=None):
    """generate_recall_record for every scene of a batch, in one launch and without a host read.
    pred_boxes (B, K, >= 7) float32 post_processing's padded boxes, num_pred (B) int the valid rows of each scene,
    gt_boxes (B, T, >= 7) float32 batch_dict['gt_boxes'], thresh_list RECALL_THRESH_LIST.  ADDS the kept GT rows and the
    rows recalled at each threshold to counters ((1 + len(thresh_list)) int64 [gt, rcnn_<t>...], zeros when None) and
    returns them; max_iou (B, T) float32, optional, receives each kept row's best IoU (0 without predictions)."""
    for name, x in (("pred_boxes", pred_boxes), ("gt_boxes", gt_boxes)):
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != F32 or x.dim() != 3 or x.shape[-1] < 7:
            raise TypeError("%s must be a (B, N, >= 7) float32 device tensor" % name)
    B, K = pred_boxes.shape[0], pred_boxes.shape[1]
    T, C = gt_boxes.shape[1], gt_boxes.shape[2]
    if gt_boxes.shape[0] != B or not isinstance(num_pred, torch.Tensor) or num_pred.numel() != B:
        raise ValueError("pred_boxes, num_pred and gt_boxes disagree on the batch size")
    if not num_pred.is_cuda or num_pred.dtype not in (torch.int32, torch.int64):
        raise TypeError("num_pred must be an int32 / int64 device tensor")
    thr, n = _thresh_array(thresh_list)
    dev = pred_boxes.device
    if counters is None:
        counters = torch.zeros(1 + n, dtype=torch.int64, device=dev)
    elif counters.numel() != 1 + n:
        raise ValueError("counters need %d elements" % (1 + n))
    boxes = pred_boxes[..., :7].contiguous()
    num = num_pred.reshape(B).to(I32).contiguous()
    gt = gt_boxes.contiguous()
    mi = None
    if max_iou is not None:
        if max_iou.numel() != B * T:
            raise ValueError("max_iou needs %d elements" % (B * T))
        mi = _chk(max_iou, "max_iou", F32)
    _call("pda_recall_record", boxes, _chk(boxes, "pred_boxes", F32), _chk(num, "num_pred", I32), _chk(gt, "gt_boxes", F32), C,
          thr, n, _chk(counters, "counters", torch.int64), mi, B, K, T)
    return counters


class RecallRecorder:
    """eval_one_epoch's recall over a whole eval loop, on the device (eval_utils.py:12-20, 111-118).  add() launches one
    kernel per batch and reads nothing back, so a loop that feeds OnceEvaluator / KittiEvaluator stays free of host
    reads and add() can be captured in a graph; compute() reads the counters once."""

    def __init__(self, thresh_list, device='cuda', enabled=True):
        self.thresh_list = list(thresh_list)
        _thresh_array(self.thresh_list)
        self.enabled = bool(enabled)
        self.counters = torch.zeros(1 + len(self.thresh_list), dtype=torch.int64, device=device)

    @classmethod
    def from_config(cls, post_process_cfg, device='cuda'):
        """MODEL.POST_PROCESSING: RECALL_THRESH_LIST, and RECALL_MODE (default 'normal'); with any other mode the
        reference records no recall, and neither does the recorder (its sums stay 0)."""
        return cls(post_process_cfg['RECALL_THRESH_LIST'], device,
                   enabled=post_process_cfg.get('RECALL_MODE', 'normal') == 'normal')

    def reset(self):
        self.counters.zero_()

    def add(self, padded, gt_boxes):
        """post_processing's padded tensors (pred_boxes, num_pred) and the batch's gt_boxes (B, max_gt, >= 7), or None
        for a batch without GT (adds nothing, as in the reference)."""
        if self.enabled and gt_boxes is not None:
            recall_record(padded['pred_boxes'], padded['num_pred'], gt_boxes, self.thresh_list, self.counters)

    def compute(self):
        """(metric, ret_dict): statistics_info's sums gt_num, recall_roi_<t>, recall_rcnn_<t>, and eval_one_epoch's
        recall/roi_<t>, recall/rcnn_<t> = sum / max(gt_num, 1)."""
        h = self.counters.tolist()                      # the one read
        metric = {'gt_num': int(h[0])}
        ret = {}
        for i, t in enumerate(self.thresh_list):
            metric['recall_roi_%s' % str(t)] = 0
            metric['recall_rcnn_%s' % str(t)] = int(h[1 + i])
        for t in self.thresh_list:
            ret['recall/roi_%s' % str(t)] = metric['recall_roi_%s' % str(t)] / max(metric['gt_num'], 1)
            ret['recall/rcnn_%s' % str(t)] = metric['recall_rcnn_%s' % str(t)] / max(metric['gt_num'], 1)
        return metric, ret
