"""ONCE evaluation on the device: AP per class and distance band, as the reference's
pcdet/datasets/once/once_eval/evaluation.py get_evaluation_results.

csrc/once_eval.hip runs the whole evaluation: the per-frame 3D IoU blocks (pda_once_eval_iou), accumulate_scores for
every (frame, class, level) (pda_once_eval_accumulate), get_thresholds and compute_statistics (pda_once_eval_match).
Between the last two, each (class, level) segment of TP scores is sorted in descending order with torch.sort.  The
inputs go up in one copy and the tp / fp / fn counts come back in one; the AP composition then runs here in float64
numpy in the reference's order, so ret_dict follows the reference's arithmetic on the same counts.

Names are data: every name seen gets an id, and a small accept[class][name] table says which evaluated class takes it
(superclass mode: 'Vehicle' takes every name but Pedestrian and Cyclist).  GT boxes are evaluated as float64 and
predictions as float32, the dtypes the reference sees from its infos and from the model.
"""
import ctypes

import numpy as np
import torch

from . import _lib, eval_common as ec
from .pointnet2_batch_cuda import _call

IOU_THRESHOLDS = {'Car': 0.7, 'Bus': 0.7, 'Truck': 0.7, 'Pedestrian': 0.3, 'Cyclist': 0.5}
SUPERCLASS_IOU_THRESHOLDS = {'Vehicle': 0.7, 'Pedestrian': 0.3, 'Cyclist': 0.5}
DIFFICULTY_MODES = {'Overall&Distance': (0, ('overall', '0-30m', '30-50m', '50m-inf')),
                    'Overall': (1, ('overall',)),
                    'Distance': (2, ('0-30m', '30-50m', '50m-inf'))}
_VEHICLES = ('Car', 'Bus', 'Truck')
_NOT_VEHICLE = ('Pedestrian', 'Cyclist')
MAX_NAMES = 64
MAX_PRED = 4096
ptr = ec.ptr


def eval_classes(classes, use_superclass):
    """The evaluated class list: with the superclass, Car/Bus/Truck (all or none) become 'Vehicle', first."""
    classes = list(classes)
    if not use_superclass:
        return classes
    if any(c in classes for c in _VEHICLES):
        assert all(c in classes for c in _VEHICLES), "Car/Bus/Truck must all exist for vehicle detection"
    return ['Vehicle'] + [c for c in classes if c not in _VEHICLES]


def accept_table(classes, names, use_superclass):
    """uint8 (len(classes), len(names)): 1 where the evaluated class takes the name (filter_data's rejection rule)."""
    t = np.zeros((len(classes), len(names)), np.uint8)
    for c, cls in enumerate(classes):
        for n, name in enumerate(names):
            if use_superclass and cls == 'Vehicle':
                t[c, n] = name not in _NOT_VEHICLE
            else:
                t[c, n] = name == cls
    return t


def _names(anno):
    return np.asarray(anno['name']).astype(str).reshape(-1)


def _rows7(boxes, n, dtype):
    b = np.asarray(boxes, dtype)
    return b.reshape(n, b.size // n)[:, :7] if n else np.zeros((0, 7), dtype)


class _Frames:
    """Device GT and predictions of a frame set, in the pda_once_frames_t layout."""

    def __init__(self, gt_boxes, gt_name, gt_offsets, n_gt, pred_boxes, pred_score, pred_name, pred_start, pred_count,
                 pred_rows, max_pred):
        self.gt_boxes, self.gt_name, self.gt_offsets, self.n_gt = gt_boxes, gt_name, gt_offsets, n_gt
        self.pred_boxes, self.pred_score, self.pred_name = pred_boxes, pred_score, pred_name
        self.pred_start, self.pred_count, self.max_pred = pred_start, pred_count, max_pred
        self.pred_rows = pred_rows                       # host: the IoU row length of each frame (count or capacity)
        self.iou_start_host, self.iou_total = ec.pair_offsets(n_gt, pred_rows)

    def struct(self, iou_start):
        return _lib.OnceFrames(ptr(self.gt_boxes), ptr(self.gt_name), ptr(self.gt_offsets), ptr(self.pred_boxes),
                               ptr(self.pred_score), ptr(self.pred_name), ptr(self.pred_start), ptr(self.pred_count),
                               ptr(iou_start), int(self.gt_boxes.shape[0]), int(self.pred_score.shape[0]),
                               self.iou_total, len(self.n_gt), int(self.n_gt.max(initial=0)), int(self.max_pred))


class _Plan:
    """Classes, thresholds and the accept table of one evaluation setting."""

    def __init__(self, classes, names, use_superclass, iou_thresholds, num_pr_points, difficulty_mode):
        if difficulty_mode not in DIFFICULTY_MODES:
            raise ValueError("difficulty mode %r is not supported" % (difficulty_mode,))
        if iou_thresholds is None:
            iou_thresholds = SUPERCLASS_IOU_THRESHOLDS if use_superclass else IOU_THRESHOLDS
        self.classes = eval_classes(classes, use_superclass)
        self.thr = np.array([float(iou_thresholds[c]) for c in self.classes], np.float64)
        if (self.thr < 0).any():
            raise ValueError("IoU thresholds must be >= 0")
        self.mode, self.diff_types = DIFFICULTY_MODES[difficulty_mode]
        self.num_pr_points = int(num_pr_points)
        self.accept = np.ascontiguousarray(accept_table(self.classes, names, use_superclass))
        self.n_names = len(names)
        C, D, P1 = len(self.classes), len(self.diff_types), self.num_pr_points + 1
        self.layout = ec.ResultLayout("ONCE", [('counts', np.int64, (C, D, P1, 3)), ('n_thresholds', np.int64, (C, D)),
                                               ('num_valid_gt', np.int64, (C, D)),
                                               ('thresholds', np.float64, (C, D, P1))])


def _run_stages(fr, plan, with_heading, iou=None):
    """IoU (unless given), accumulate, sort, match on the current stream.  Returns the device iou buffer and the one
    int64 device result buffer of plan.layout."""
    dev = fr.gt_offsets.device
    T = len(plan.classes) * len(plan.diff_types)
    res = plan.layout.alloc(dev)
    out = {k: v.data_ptr() for k, v in plan.layout.device_views(res).items()}
    st = ctypes.byref(fr.struct(fr.iou_start))
    if iou is None:
        iou = torch.empty(max(fr.iou_total, 1), dtype=torch.float64, device=dev)
        _call("pda_once_eval_iou", res, st, 1 if with_heading else 0, iou.data_ptr(), out['status'])
    n_gt_total = int(fr.gt_boxes.shape[0])
    ws = ec.workspace("pda_once_eval_workspace_bytes", (len(fr.n_gt), n_gt_total, T), "ONCE evaluation: sizes out of range", dev)
    thr_c = (ctypes.c_double * len(plan.thr))(*plan.thr.tolist())
    acc = plan.accept.ctypes.data
    args = (acc, len(plan.classes), plan.n_names, thr_c, plan.mode)
    _call("pda_once_eval_accumulate", res, st, iou.data_ptr(), *args, out['num_valid_gt'], out['status'], ws.data_ptr())
    seg = ws[:T * n_gt_total * 4].view(torch.float32).view(T, n_gt_total)
    ordered = torch.sort(seg, dim=1, descending=True).values if n_gt_total else seg
    _call("pda_once_eval_match", res, st, iou.data_ptr(), *args, plan.num_pr_points,
          ordered.data_ptr() if n_gt_total else None, out['num_valid_gt'], out['thresholds'], out['n_thresholds'],
          out['counts'], out['status'], ws.data_ptr())
    return iou, res


def _read(res, plan):
    """The one device-to-host copy, split into counts (C, D, P+1, 3), n_thresholds (C, D), num_valid_gt (C, D) and
    thresholds (C, D, P+1); raises on a status bit."""
    return plan.layout.host_views(res.cpu().numpy())


def compose(out, plan, print_ok=False):
    """(ret_str, ret_dict) from the read-back counts, in the reference's float64 order: precision per threshold, its
    running maximum over the later thresholds, AP = the sequential sum of precision[1:] / num_pr_points * 100."""
    C, D, P = len(plan.classes), len(plan.diff_types), plan.num_pr_points
    precision = np.zeros((C, D, P + 1))
    for c in range(C):
        for d in range(D):
            nt = int(out['n_thresholds'][c, d])
            cm = out['counts'][c, d, :nt].astype(np.float64)
            with np.errstate(divide='ignore', invalid='ignore'):
                precision[c, d, :nt] = cm[:, 0] / (cm[:, 0] + cm[:, 1])
            for t in range(nt):
                precision[c, d, t] = np.max(precision[c, d, t:], axis=-1)
    ap = 0
    for t in range(1, P + 1):
        ap += precision[..., t]
    ap = ap / P * 100
    m_ap = np.mean(ap, axis=0)
    ret_dict = {}
    lines = ['\n|AP@%-9s|' % str(P) + ''.join('%-12s|' % t for t in plan.diff_types)]
    for name, row, prefix in [(c, ap[i], 'AP_' + c) for i, c in enumerate(plan.classes)] + [('mAP', m_ap, 'AP_mean')]:
        for d, t in enumerate(plan.diff_types):
            ret_dict[prefix + '/' + t] = row[d]
        lines.append('|%-12s|' % name + ''.join('%-12.2f|' % v for v in row))
    ret_str = '\n'.join(lines) + '\n'
    if print_ok:
        print(ret_str)
    return ret_str, ret_dict


def _gt_arrays(gt_annos, vocab):
    n_gt = np.array([len(_names(a)) for a in gt_annos], np.int64)
    boxes = [_rows7(a['boxes_3d'], n, np.float64) for a, n in zip(gt_annos, n_gt)]
    boxes = np.concatenate(boxes, 0) if boxes else np.zeros((0, 7))
    names = [_names(a) for a in gt_annos]
    names = np.concatenate(names) if names else np.zeros(0, str)
    ids = np.array([vocab[n] for n in names.tolist()], np.int32)
    offs = np.zeros(len(gt_annos) + 1, np.int64)
    np.cumsum(n_gt, out=offs[1:])
    return np.ascontiguousarray(boxes), ids, offs, n_gt


def _vocab(*name_lists):
    return ec.vocab(name_lists, MAX_NAMES, "ONCE")


def frames_from_annos(gt_annos, pred_annos, vocab, device):
    """Packed device frames of a GT and prediction list (one upload)."""
    gb, gid, goffs, n_gt = _gt_arrays(gt_annos, vocab)
    n_pred = np.array([len(_names(a)) for a in pred_annos], np.int64)
    if n_pred.max(initial=0) > MAX_PRED:
        raise ValueError("ONCE evaluation supports at most %d predictions a frame" % MAX_PRED)
    pb = [_rows7(a['boxes_3d'], n, np.float32) for a, n in zip(pred_annos, n_pred)]
    pb = np.ascontiguousarray(np.concatenate(pb, 0)) if pb else np.zeros((0, 7), np.float32)
    ps = [np.asarray(a['score'], np.float32).reshape(-1) for a in pred_annos]
    ps = np.concatenate(ps) if ps else np.zeros(0, np.float32)
    pn = [_names(a) for a in pred_annos]
    pn = np.concatenate(pn) if pn else np.zeros(0, str)
    pid = np.array([vocab[n] for n in pn.tolist()], np.int32)
    fr = _Frames(None, None, None, n_gt, None, None, None, None, None, n_pred, int(n_pred.max(initial=0)))
    d = ec.upload([gb, gid, goffs, pb, ps, pid, ec.row_starts(n_pred), n_pred.astype(np.int32), fr.iou_start_host],
                  device)
    fr.gt_boxes, fr.gt_name, fr.gt_offsets, fr.pred_boxes, fr.pred_score, fr.pred_name = d[:6]
    fr.pred_start, fr.pred_count, fr.iou_start = d[6], d[7], d[8]
    return fr


def get_evaluation_results(gt_annos, pred_annos, classes, use_superclass=True, iou_thresholds=None, num_pr_points=50,
                           difficulty_mode='Overall&Distance', ap_with_heading=True, num_parts=100, print_ok=False,
                           device='cuda'):
    """The reference's get_evaluation_results on the device: returns (ret_str, ret_dict).  num_parts is accepted and
    has no effect (the reference only uses the per-frame blocks of its part matrices)."""
    assert len(gt_annos) == len(pred_annos), "the number of GT must match predictions"
    vocab = _vocab(list(classes), *[_names(a) for a in gt_annos], *[_names(a) for a in pred_annos])
    plan = _Plan(classes, list(vocab), use_superclass, iou_thresholds, num_pr_points, difficulty_mode)
    fr = frames_from_annos(gt_annos, pred_annos, vocab, torch.device(device))
    _, res = _run_stages(fr, plan, ap_with_heading)
    return compose(_read(res, plan), plan, print_ok)


def generate_prediction_dicts(batch_dict, pred_dicts, class_names, output_path=None):
    """The reference's ONCEDataset.generate_prediction_dicts: per frame {'name', 'score', 'boxes_3d', 'frame_id'}, a
    float64 zero template for a frame without predictions."""
    if output_path is not None:
        raise NotImplementedError
    annos = []
    for index, box_dict in enumerate(pred_dicts):
        scores = box_dict['pred_scores'].cpu().numpy()
        if scores.shape[0] == 0:
            anno = {'name': np.zeros(0), 'score': np.zeros(0), 'boxes_3d': np.zeros((0, 7))}
        else:
            labels = box_dict['pred_labels'].cpu().numpy()
            anno = {'name': np.array(class_names)[labels - 1], 'score': scores,
                    'boxes_3d': box_dict['pred_boxes'].cpu().numpy()}
        anno['frame_id'] = batch_dict['frame_id'][index]
        annos.append(anno)
    return annos


class OnceEvaluator:
    """Streaming ONCE evaluation for an eval loop: GT goes up once here, add_batch() keeps post_processing's padded
    device tensors without a host read, compute() runs the evaluation and reads back once."""

    def __init__(self, class_names, gt_annos, use_superclass=True, iou_thresholds=None, num_pr_points=50,
                 difficulty_mode='Overall&Distance', ap_with_heading=True, device='cuda'):
        self.class_names = list(class_names)
        self.vocab = _vocab(self.class_names, *[_names(a) for a in gt_annos])
        self.plan = _Plan(self.class_names, list(self.vocab), use_superclass, iou_thresholds, num_pr_points,
                          difficulty_mode)
        self.with_heading = ap_with_heading
        self.device = torch.device(device)
        gb, gid, goffs, self.n_gt = _gt_arrays(gt_annos, self.vocab)
        self.gt = ec.upload([gb, gid, goffs], self.device)
        self.batches = []
        self.n_frames = 0

    def add_batch(self, padded):
        """pred_boxes (B, K, >= 7), pred_scores (B, K), pred_labels (B, K) int, num_pred (B): the next B frames."""
        boxes = padded['pred_boxes'][..., :7].to(torch.float32).contiguous()
        B, K = boxes.shape[0], boxes.shape[1]
        if K > MAX_PRED:
            raise ValueError("ONCE evaluation supports at most %d predictions a frame" % MAX_PRED)
        idx = ec.label_name_ids(padded['pred_labels'], len(self.class_names))
        num = ec.clamp_num_pred(padded['num_pred'], K)
        self.batches.append((boxes.view(B * K, 7), padded['pred_scores'].to(torch.float32).reshape(B * K).contiguous(),
                             idx.reshape(B * K).contiguous(), num.reshape(B), B, K))
        self.n_frames += B

    def compute(self, print_ok=False):
        if self.n_frames != len(self.n_gt):
            raise ValueError("%d frames of predictions for %d GT frames" % (self.n_frames, len(self.n_gt)))
        empty = lambda dt, *s: torch.zeros(s, dtype=dt, device=self.device)
        cat = lambda i, dt, *s: torch.cat([b[i] for b in self.batches]) if self.batches else empty(dt, *s)
        rows = ec.padded_rows([b[4:6] for b in self.batches])
        fr = _Frames(self.gt[0], self.gt[1], self.gt[2], self.n_gt, cat(0, torch.float32, 0, 7), cat(1, torch.float32, 0),
                     cat(2, torch.int32, 0), None, cat(3, torch.int32, 0), rows, int(rows.max(initial=0)))
        fr.pred_start, fr.iou_start = ec.upload([ec.row_starts(rows), fr.iou_start_host], self.device)
        _, res = _run_stages(fr, self.plan, self.with_heading)
        return compose(_read(res, self.plan), self.plan, print_ok)
