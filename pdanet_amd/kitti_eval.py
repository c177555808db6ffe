"""KITTI evaluation on the device: bbox / BEV / 3D / AOS AP (R11 and R40), as the reference's
pcdet/datasets/kitti/kitti_object_eval_python/eval.py get_official_eval_result.

csrc/kitti_eval.hip runs the whole evaluation: the per-frame overlap blocks of the three metrics
(pda_kitti_eval_overlaps), clean_data's flags and compute_statistics_jit(compute_fp=False) for every (frame, task)
(pda_kitti_eval_first_pass), get_thresholds and compute_statistics_jit(compute_fp=True) for every (frame, task,
threshold) (pda_kitti_eval_match).  Between the last two, each task's segment of TP scores is sorted in descending order
with torch.sort.  The inputs go up in one copy and the pr table comes back in one; precision / recall / aos, get_mAP and
get_mAP_R40 then run here in float64 numpy in the reference's order.

Names are data: every name seen gets an id, and small tables say which evaluated class takes it (compared lowercased;
Van is an ignored GT of Car, Person_sitting of Pedestrian) and which id is 'DontCare' (compared as written).  Inputs
are evaluated in the dtypes of KITTI infos and of generate_prediction_dicts: GT bbox and location float32, GT
dimensions, rotation_y, alpha, truncated and occluded float64, detections float32.  Where numpy would compute in float64
because a frame of the same part (get_split_parts(n, 100)) carries float64 arrays, a per-frame mode says so.
"""
import ctypes
import io

import numpy as np
import torch

from . import _lib, eval_common as ec
from .pointnet2_batch_cuda import _call

CLASS_TO_NAME = {0: 'Car', 1: 'Pedestrian', 2: 'Cyclist', 3: 'Van', 4: 'Person_sitting', 5: 'Truck'}
NAME_TO_CLASS = {v: n for n, v in CLASS_TO_NAME.items()}
_OVERLAP_0_7 = [[0.7, 0.5, 0.5, 0.7, 0.5, 0.7]] * 3
_OVERLAP_0_5 = [[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]]
MIN_OVERLAPS = np.array([_OVERLAP_0_7, _OVERLAP_0_5])      # [setting, metric, class]
N_SAMPLE_PTS = 41
NUM_PARTS = 100
MAX_NAMES = 64
MAX_DET = 4096
CALIB_FLOATS = 33
# frame_mode bits (include/pda_train.h)
MODE_IMG_DT64, MODE_IMG_GT64, MODE_3D_DT64, MODE_DC_DT64 = 1, 2, 4, 8
ptr = ec.ptr


def class_ids(current_classes):
    """get_official_eval_result's class list: ids or names of CLASS_TO_NAME."""
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    ids = [NAME_TO_CLASS[c] if isinstance(c, str) else int(c) for c in current_classes]
    for c in ids:
        if c not in CLASS_TO_NAME:
            raise KeyError(c)
    return ids


def name_tables(ids, names):
    """gt_class (C, N) int8, dt_class (C, N) uint8, dontcare (N) uint8 of clean_data for class ids over a name list."""
    gt = np.full((len(ids), len(names)), -1, np.int8)
    dt = np.zeros((len(ids), len(names)), np.uint8)
    for c, cid in enumerate(ids):
        cur = CLASS_TO_NAME[cid].lower()
        for n, name in enumerate(names):
            low = name.lower()
            if low == cur:
                gt[c, n] = 1
                dt[c, n] = 1
            elif (cur == 'pedestrian' and low == 'person_sitting') or (cur == 'car' and low == 'van'):
                gt[c, n] = 0
    dc = np.array([name == 'DontCare' for name in names], np.uint8)
    return gt, dt, dc


def split_parts(num, num_part=NUM_PARTS):
    """eval.get_split_parts."""
    same, remain = num // num_part, num % num_part
    if same == 0:
        return [num]
    return [same] * num_part + ([remain] if remain else [])


def frame_modes(gt_annos, dt_annos, num_parts=NUM_PARTS):
    """The per-frame dtype bits: what numpy computes in when it concatenates the frame's part."""
    f64 = lambda arrays: np.result_type(*arrays) == np.float64 if arrays else False
    modes = np.zeros(len(gt_annos), np.int32)
    s = 0
    for n in split_parts(len(gt_annos), num_parts):
        g, d = gt_annos[s:s + n], dt_annos[s:s + n]
        m = 0
        if f64([np.asarray(a['bbox']) for a in d]):
            m |= MODE_IMG_DT64
        if f64([np.asarray(a['bbox']) for a in g]):
            m |= MODE_IMG_GT64
        if f64([np.asarray(a[k]) for a in d for k in ('location', 'dimensions', 'rotation_y')]):
            m |= MODE_3D_DT64
        if f64([np.asarray(a[k]) for a in d for k in ('bbox', 'alpha', 'score')]):
            m |= MODE_DC_DT64
        modes[s:s + n] = m
        s += n
    return modes


def _names(anno):
    return [str(n) for n in np.asarray(anno['name']).reshape(-1).tolist()]


def _vocab(*name_lists):
    return ec.vocab(name_lists, MAX_NAMES, "KITTI")


def _col(annos, key, dtype, width=None):
    parts = []
    for a in annos:
        v = np.asarray(a[key], dtype)
        parts.append(v.reshape(-1, width) if width else v.reshape(-1))
    if parts:
        return np.ascontiguousarray(np.concatenate(parts, 0))
    return np.zeros((0, width) if width else 0, dtype)


def gt_arrays(gt_annos, vocab):
    """Host GT columns in the device layout: bbox, loc, dims, ry, alpha, trunc, occ, name ids, offsets; and n_gt."""
    n_gt = np.array([len(_names(a)) for a in gt_annos], np.int64)
    offs = np.zeros(len(gt_annos) + 1, np.int64)
    np.cumsum(n_gt, out=offs[1:])
    names = [n for a in gt_annos for n in _names(a)]
    ids = np.array([vocab[n] for n in names], np.int32)
    cols = [_col(gt_annos, 'bbox', np.float32, 4), _col(gt_annos, 'location', np.float32, 3),
            _col(gt_annos, 'dimensions', np.float64, 3), _col(gt_annos, 'rotation_y', np.float64),
            _col(gt_annos, 'alpha', np.float64), _col(gt_annos, 'truncated', np.float64),
            _col(gt_annos, 'occluded', np.float64), ids, offs]
    return cols, n_gt


class _Frames:
    """Device GT and detections of a frame set, in the pda_kitti_frames_t layout."""

    def __init__(self, gt, n_gt, dt, dt_rows, max_det, dt_start=None, dt_count=None, ov_start=None, mode=None):
        self.gt, self.n_gt = gt, n_gt                    # device: bbox, loc, dims, ry, alpha, trunc, occ, name, offsets
        self.dt = dt                                     # device: bbox (R, 4), box (R, 7), alpha, score, name
        self.dt_rows, self.max_det = dt_rows, max_det    # host: the overlap row length of each frame
        self.dt_start, self.dt_count, self.ov_start, self.mode = dt_start, dt_count, ov_start, mode
        self.ov_start_host, self.ov_total = ec.pair_offsets(n_gt, dt_rows)

    def struct(self):
        return _lib.KittiFrames(*[ptr(t) for t in self.gt], *[ptr(t) for t in self.dt], ptr(self.dt_start),
                                ptr(self.dt_count), ptr(self.ov_start), ptr(self.mode), int(self.gt[0].shape[0]),
                                int(self.dt[3].shape[0]), self.ov_total, len(self.n_gt), int(self.n_gt.max(initial=0)),
                                int(self.max_det))


def frames_from_annos(gt_annos, dt_annos, vocab, device, num_parts=NUM_PARTS):
    """Packed device frames of a GT and detection list (one upload)."""
    gcols, n_gt = gt_arrays(gt_annos, vocab)
    n_dt = np.array([len(_names(a)) for a in dt_annos], np.int64)
    if n_dt.max(initial=0) > MAX_DET:
        raise ValueError("KITTI evaluation supports at most %d detections a frame" % MAX_DET)
    box = np.concatenate([_col(dt_annos, 'location', np.float32, 3), _col(dt_annos, 'dimensions', np.float32, 3),
                          _col(dt_annos, 'rotation_y', np.float32)[:, None]], 1)
    dcols = [_col(dt_annos, 'bbox', np.float32, 4), np.ascontiguousarray(box), _col(dt_annos, 'alpha', np.float32),
             _col(dt_annos, 'score', np.float32),
             np.array([vocab[n] for a in dt_annos for n in _names(a)], np.int32)]
    fr = _Frames(None, n_gt, None, n_dt, int(n_dt.max(initial=0)))
    d = ec.upload(gcols + dcols + [ec.row_starts(n_dt), n_dt.astype(np.int32), fr.ov_start_host,
                                   frame_modes(gt_annos, dt_annos, num_parts)], device)
    fr.gt, fr.dt = d[:9], d[9:14]
    fr.dt_start, fr.dt_count, fr.ov_start, fr.mode = d[14:18]
    return fr


class _Plan:
    """Class ids, name tables and min_overlaps of one evaluation."""

    def __init__(self, current_classes, names):
        self.ids = class_ids(current_classes)
        self.C = len(self.ids)
        self.gt_class, self.dt_class, self.dontcare = (np.ascontiguousarray(t) for t in name_tables(self.ids, names))
        self.min_overlaps = np.ascontiguousarray(MIN_OVERLAPS[:, :, self.ids])   # (2, 3, C)
        self.n_names = max(len(names), 1)
        if len(names) == 0:
            self.gt_class = np.full((self.C, 1), -1, np.int8)
            self.dt_class = np.zeros((self.C, 1), np.uint8)
            self.dontcare = np.zeros(1, np.uint8)
        C, P = self.C, N_SAMPLE_PTS
        self.layout = ec.ResultLayout("KITTI", [('counts', np.int64, (3, C, 3, 2, P, 3)),
                                                ('n_thresholds', np.int64, (3, C, 3, 2)),
                                                ('num_valid_gt', np.int64, (C, 3)),
                                                ('thresholds', np.float64, (3, C, 3, 2, P)),
                                                ('similarity', np.float64, (C, 3, 2, P))])

    @property
    def T(self):
        return 18 * self.C


def _run_stages(fr, plan, compute_aos, overlaps=None):
    """Overlaps (unless given), first pass, sort, match on the current stream.  Returns the device overlaps, the flags and
    the one int64 device result buffer of plan.layout."""
    dev = fr.gt[8].device
    T, C = plan.T, plan.C
    res = plan.layout.alloc(dev)
    out = {k: v.data_ptr() for k, v in plan.layout.device_views(res).items()}
    st = ctypes.byref(fr.struct())
    if overlaps is None:
        overlaps = torch.empty(max(3 * fr.ov_total, 1), dtype=torch.float64, device=dev)
        _call("pda_kitti_eval_overlaps", res, st, overlaps.data_ptr(), out['status'])
    n_gt_total, det_cap = int(fr.gt[0].shape[0]), int(fr.dt[3].shape[0])
    ws = ec.workspace("pda_kitti_eval_workspace_bytes", (len(fr.n_gt), n_gt_total, det_cap, C),
                      "KITTI evaluation: sizes out of range", dev)
    flags = torch.empty(3 * C * (n_gt_total + det_cap) + 1, dtype=torch.int8, device=dev)
    gt_flags, dt_flags = flags[:3 * C * n_gt_total], flags[3 * C * n_gt_total:-1]
    mo = (ctypes.c_double * plan.min_overlaps.size)(*plan.min_overlaps.reshape(-1).tolist())
    tables = (plan.C, plan.n_names, plan.gt_class.ctypes.data, plan.dt_class.ctypes.data, plan.dontcare.ctypes.data, mo)
    _call("pda_kitti_eval_first_pass", res, st, overlaps.data_ptr(), *tables, ptr(gt_flags), ptr(dt_flags),
          out['num_valid_gt'], out['status'], ws.data_ptr())
    seg = ws[:T * n_gt_total * 4].view(torch.float32).view(T, n_gt_total)
    ordered = torch.sort(seg, dim=1, descending=True).values if n_gt_total else seg
    _call("pda_kitti_eval_match", res, st, overlaps.data_ptr(), *tables, 1 if compute_aos else 0, ptr(gt_flags),
          ptr(dt_flags), ordered.data_ptr() if n_gt_total else None, out['num_valid_gt'], out['thresholds'],
          out['n_thresholds'], out['counts'], out['similarity'], out['status'], ws.data_ptr())
    return overlaps, (gt_flags, dt_flags), res


def _read(res, plan):
    """The one device-to-host copy of _run_stages' result buffer: counts (3, C, 3, 2, 41, 3), n_thresholds (3, C, 3, 2),
    num_valid_gt (C, 3), thresholds (3, C, 3, 2, 41) and similarity (C, 3, 2, 41); raises on a status bit."""
    return plan.layout.host_views(res.cpu().numpy())


def _eval_metric(out, metric, compute_aos):
    """eval_class's precision / recall / aos of one metric from the pr table, in the reference's float64 order."""
    C = out['counts'].shape[1]
    shape = (C, 3, 2, N_SAMPLE_PTS)
    precision, recall, aos = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        for m in range(C):
            for l in range(3):
                for k in range(2):
                    nt = int(out['n_thresholds'][metric, m, l, k])
                    pr = np.zeros([nt, 4])
                    pr[:, :3] = out['counts'][metric, m, l, k, :nt]
                    if compute_aos:
                        pr[:, 3] = out['similarity'][m, l, k, :nt]
                    for i in range(nt):
                        recall[m, l, k, i] = pr[i, 0] / (pr[i, 0] + pr[i, 2])
                        precision[m, l, k, i] = pr[i, 0] / (pr[i, 0] + pr[i, 1])
                        if compute_aos:
                            aos[m, l, k, i] = pr[i, 3] / (pr[i, 0] + pr[i, 1])
                    for i in range(nt):
                        precision[m, l, k, i] = np.max(precision[m, l, k, i:], axis=-1)
                        recall[m, l, k, i] = np.max(recall[m, l, k, i:], axis=-1)
                        if compute_aos:
                            aos[m, l, k, i] = np.max(aos[m, l, k, i:], axis=-1)
    return {"recall": recall, "precision": precision, "orientation": aos}


def get_mAP(prec):
    sums = 0
    for i in range(0, prec.shape[-1], 4):
        sums = sums + prec[..., i]
    return sums / 11 * 100


def get_mAP_R40(prec):
    sums = 0
    for i in range(1, prec.shape[-1]):
        sums = sums + prec[..., i]
    return sums / 40 * 100


def _line(value):
    s = io.StringIO()
    print(value, file=s)
    return s.getvalue()


def compose(out, plan, compute_aos, PR_detail_dict=None):
    """(result, ret_dict) of get_official_eval_result from the read-back table (do_eval and the report)."""
    rets = [_eval_metric(out, m, compute_aos and m == 0) for m in range(3)]
    mAP = [get_mAP(r["precision"]) for r in rets]
    mAP40 = [get_mAP_R40(r["precision"]) for r in rets]
    mAPaos = get_mAP(rets[0]["orientation"]) if compute_aos else None
    mAPaos40 = get_mAP_R40(rets[0]["orientation"]) if compute_aos else None
    if PR_detail_dict is not None:
        PR_detail_dict['bbox'] = rets[0]['precision']
        if compute_aos:
            PR_detail_dict['aos'] = rets[0]['orientation']
        PR_detail_dict['bev'] = rets[1]['precision']
        PR_detail_dict['3d'] = rets[2]['precision']
    (bb, bev, d3), (bb40, bev40, d340) = mAP, mAP40
    mo = plan.min_overlaps
    result, ret_dict = '', {}
    for j, curcls in enumerate(plan.ids):
        name = CLASS_TO_NAME[curcls]
        for i in range(mo.shape[0]):
            result += _line(f"{name} " "AP@{:.2f}, {:.2f}, {:.2f}:".format(*mo[i, :, j]))
            result += _line(f"bbox AP:{bb[j, 0, i]:.4f}, {bb[j, 1, i]:.4f}, {bb[j, 2, i]:.4f}")
            result += _line(f"bev  AP:{bev[j, 0, i]:.4f}, {bev[j, 1, i]:.4f}, {bev[j, 2, i]:.4f}")
            result += _line(f"3d   AP:{d3[j, 0, i]:.4f}, {d3[j, 1, i]:.4f}, {d3[j, 2, i]:.4f}")
            if compute_aos:
                result += _line(f"aos  AP:{mAPaos[j, 0, i]:.2f}, {mAPaos[j, 1, i]:.2f}, {mAPaos[j, 2, i]:.2f}")
            result += _line(f"{name} " "AP_R40@{:.2f}, {:.2f}, {:.2f}:".format(*mo[i, :, j]))
            result += _line(f"bbox AP:{bb40[j, 0, i]:.4f}, {bb40[j, 1, i]:.4f}, {bb40[j, 2, i]:.4f}")
            result += _line(f"bev  AP:{bev40[j, 0, i]:.4f}, {bev40[j, 1, i]:.4f}, {bev40[j, 2, i]:.4f}")
            result += _line(f"3d   AP:{d340[j, 0, i]:.4f}, {d340[j, 1, i]:.4f}, {d340[j, 2, i]:.4f}")
            if compute_aos:
                result += _line(f"aos  AP:{mAPaos40[j, 0, i]:.2f}, {mAPaos40[j, 1, i]:.2f}, {mAPaos40[j, 2, i]:.2f}")
                if i == 0:
                    for d, diff in enumerate(('easy', 'moderate', 'hard')):
                        ret_dict['%s_aos/%s_R40' % (name, diff)] = mAPaos40[j, d, 0]
            if i == 0:
                for key, arr in (('3d', d340), ('bev', bev40), ('image', bb40)):
                    for d, diff in enumerate(('easy', 'moderate', 'hard')):
                        ret_dict['%s_%s/%s_R40' % (name, key, diff)] = arr[j, d, 0]
    return result, ret_dict


def compute_aos_of(dt_annos):
    """The reference's test: the first detection frame that is not empty decides, by alpha[0] != -10."""
    for anno in dt_annos:
        if np.asarray(anno['alpha']).shape[0] != 0:
            return bool(np.asarray(anno['alpha'])[0] != -10)
    return False


def get_official_eval_result(gt_annos, dt_annos, current_classes, PR_detail_dict=None, device='cuda'):
    """The reference's get_official_eval_result on the device: returns (result, ret_dict)."""
    assert len(gt_annos) == len(dt_annos)
    plan_ids = class_ids(current_classes)
    vocab = _vocab([CLASS_TO_NAME[c] for c in plan_ids], *[_names(a) for a in gt_annos], *[_names(a) for a in dt_annos])
    plan = _Plan(plan_ids, list(vocab))
    compute_aos = compute_aos_of(dt_annos)
    fr = frames_from_annos(gt_annos, dt_annos, vocab, torch.device(device))
    _, _, res = _run_stages(fr, plan, compute_aos)
    return compose(_read(res, plan), plan, compute_aos, PR_detail_dict)


def _calib_row(calib):
    get = (lambda k: calib[k]) if isinstance(calib, dict) else (lambda k: getattr(calib, k))
    v2c = get('Tr_velo2cam') if isinstance(calib, dict) else get('V2C')
    return np.concatenate([np.asarray(get('P2'), np.float32).reshape(12)[:12], np.asarray(get('R0'), np.float32).reshape(9),
                           np.asarray(v2c, np.float32).reshape(12)])


def calib_matrix(calibs):
    """(n, 33) float32 rows P2 | R0 | V2C of Calibration objects (or their dicts)."""
    return np.ascontiguousarray(np.stack([_calib_row(c) for c in calibs]) if calibs else np.zeros((0, CALIB_FLOATS),
                                                                                                  np.float32))


def convert_predictions(boxes, frame_idx, calib, image_shape, rows_per_frame=0):
    """Device lidar boxes (n, >= 7) -> (camera boxes (n, 7), image boxes (n, 4), alpha (n)), all float32 on the device.
    frame_idx (n) int32 or None (then frame = row // rows_per_frame); calib (F, 33) float32; image_shape (F, 2) int32."""
    n = boxes.shape[0]
    dev = boxes.device
    boxes = boxes.to(torch.float32).contiguous()
    out = torch.empty(n * 12 + 1, dtype=torch.float32, device=dev)
    cam, bbox, alpha = out[:7 * n].view(n, 7), out[7 * n:11 * n].view(n, 4), out[11 * n:12 * n]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _call("pda_kitti_eval_predictions", out, ptr(boxes), n, int(boxes.shape[1]) if n else 7, int(rows_per_frame),
          ptr(frame_idx), ptr(calib), ptr(image_shape), int(calib.shape[0]), ptr(cam), ptr(bbox), ptr(alpha),
          status.data_ptr())
    return cam, bbox, alpha, status


def _template(n):
    return {'name': np.zeros(n), 'truncated': np.zeros(n), 'occluded': np.zeros(n), 'alpha': np.zeros(n),
            'bbox': np.zeros([n, 4]), 'dimensions': np.zeros([n, 3]), 'location': np.zeros([n, 3]),
            'rotation_y': np.zeros(n), 'score': np.zeros(n), 'boxes_lidar': np.zeros([n, 7])}


def generate_prediction_dicts(batch_dict, pred_dicts, class_names, output_path=None):
    """The reference's KittiDataset.generate_prediction_dicts: per frame name, truncated, occluded, alpha, bbox,
    dimensions, location, rotation_y, score, boxes_lidar and frame_id; batch_dict carries 'calib' (objects with P2, R0,
    V2C, or their dicts) and 'image_shape' per frame.  The geometry runs in one launch and comes back in one read."""
    if output_path is not None:
        raise NotImplementedError
    counts = [int(d['pred_scores'].shape[0]) for d in pred_dicts]
    live = [i for i, c in enumerate(counts) if c]
    conv = None
    if live:
        dev = pred_dicts[live[0]]['pred_boxes'].device
        boxes = torch.cat([pred_dicts[i]['pred_boxes'][:, :7].to(torch.float32) for i in live])
        fidx = torch.cat([torch.full((counts[i],), k, dtype=torch.int32) for k, i in enumerate(live)]).to(dev)
        calib = torch.from_numpy(calib_matrix([batch_dict['calib'][i] for i in live])).to(dev)
        shapes = np.stack([np.asarray(torch.as_tensor(batch_dict['image_shape'][i]).cpu()).reshape(2) for i in live])
        shapes = torch.from_numpy(shapes.astype(np.int32)).to(dev)
        cam, bbox, alpha, status = convert_predictions(boxes, fidx, calib, shapes)
        h = torch.cat([cam.reshape(-1), bbox.reshape(-1), alpha, status.view(torch.float32)]).cpu().numpy()
        n = boxes.shape[0]
        if int(h[-1:].view(np.int32)[0]):
            raise RuntimeError("KITTI prediction conversion: frame index out of range")
        conv = h[:7 * n].reshape(n, 7), h[7 * n:11 * n].reshape(n, 4), h[11 * n:12 * n]
    annos, row = [], 0
    for index, box_dict in enumerate(pred_dicts):
        c = counts[index]
        anno = _template(c)
        if c:
            cam, bbox, alpha = conv[0][row:row + c], conv[1][row:row + c], conv[2][row:row + c]
            row += c
            labels = box_dict['pred_labels'].cpu().numpy()
            anno['name'] = np.array(class_names)[labels - 1]
            anno['alpha'] = alpha.copy()
            anno['bbox'] = bbox.copy()
            anno['dimensions'] = cam[:, 3:6].copy()
            anno['location'] = cam[:, 0:3].copy()
            anno['rotation_y'] = cam[:, 6].copy()
            anno['score'] = box_dict['pred_scores'].cpu().numpy()
            anno['boxes_lidar'] = box_dict['pred_boxes'].cpu().numpy()
        anno['frame_id'] = batch_dict['frame_id'][index]
        annos.append(anno)
    return annos


class KittiEvaluator:
    """Streaming KITTI evaluation for an eval loop: GT goes up once here, add_batch() converts post_processing's padded
    device tensors on the device without a host read, compute() runs the evaluation and reads back once.  A frame's
    detections are those of generate_prediction_dicts, so AOS is evaluated unless every frame is empty."""

    def __init__(self, class_names, gt_annos, current_classes=None, device='cuda'):
        self.class_names = list(class_names)
        self.ids = class_ids(self.class_names if current_classes is None else current_classes)
        self.vocab = _vocab(self.class_names, [CLASS_TO_NAME[c] for c in self.ids], *[_names(a) for a in gt_annos])
        self.plan = _Plan(self.ids, list(self.vocab))
        self.device = torch.device(device)
        gcols, self.n_gt = gt_arrays(gt_annos, self.vocab)
        self.gt = ec.upload(gcols, self.device)
        self.gt_bbox64 = [np.asarray(a['bbox']).dtype == np.float64 for a in gt_annos]
        self.batches = []
        self.n_frames = 0

    def add_batch(self, padded, calib_mats, image_shape):
        """pred_boxes (B, K, >= 7), pred_scores (B, K), pred_labels (B, K) int, num_pred (B): the next B frames; calib_mats
        (B, 33) float32 device rows P2 | R0 | V2C (calib_matrix), image_shape (B, 2) (H, W) device."""
        boxes = padded['pred_boxes'][..., :7].to(torch.float32).contiguous()
        B, K = boxes.shape[0], boxes.shape[1]
        if K > MAX_DET:
            raise ValueError("KITTI evaluation supports at most %d detections a frame" % MAX_DET)
        calib = calib_mats.to(self.device, torch.float32).reshape(B, CALIB_FLOATS).contiguous()
        shape = image_shape.to(self.device, torch.int32).reshape(B, 2).contiguous()
        cam, bbox, alpha, status = convert_predictions(boxes.view(B * K, 7), None, calib, shape, rows_per_frame=max(K, 1))
        idx = ec.label_name_ids(padded['pred_labels'], len(self.class_names))
        num = ec.clamp_num_pred(padded['num_pred'], K)
        self.batches.append((bbox, cam, alpha, padded['pred_scores'].to(torch.float32).reshape(B * K).contiguous(),
                             idx.reshape(B * K).contiguous(), num.reshape(B), status, B, K))
        self.n_frames += B

    def compute(self, PR_detail_dict=None):
        if self.n_frames != len(self.n_gt):
            raise ValueError("%d frames of detections for %d GT frames" % (self.n_frames, len(self.n_gt)))
        dev = self.device
        empty = lambda dt, *s: torch.zeros(s, dtype=dt, device=dev)
        cat = lambda i, dt, *s: torch.cat([b[i] for b in self.batches]) if self.batches else empty(dt, *s)
        rows = ec.padded_rows([b[7:9] for b in self.batches])
        dt = [cat(0, torch.float32, 0, 4), cat(1, torch.float32, 0, 7), cat(2, torch.float32, 0),
              cat(3, torch.float32, 0), cat(4, torch.int32, 0)]
        fr = _Frames(self.gt, self.n_gt, dt, rows, int(rows.max(initial=0)))
        # generate_prediction_dicts gives a frame without detections float64 templates, which make its part float64;
        # the other frames are the conversion's float32.  Decided on the device from the counts (no read).
        parts = split_parts(len(self.n_gt))
        part_of = np.repeat(np.arange(len(parts)), parts).astype(np.int64)
        gt_mode = np.zeros(len(self.n_gt), np.int32)
        for p in range(len(parts)):
            if any(np.asarray(self.gt_bbox64)[part_of == p]):
                gt_mode[part_of == p] = MODE_IMG_GT64
        fr.dt_start, fr.ov_start, gt_mode_d, part_d = ec.upload(
            [ec.row_starts(rows), fr.ov_start_host, gt_mode, part_of], dev)
        fr.dt_count = cat(5, torch.int32, 0)
        empty_part = torch.zeros(len(parts), dtype=torch.int32, device=dev).scatter_reduce_(
            0, part_d, (fr.dt_count == 0).to(torch.int32), reduce='amax')
        dt64 = MODE_IMG_DT64 | MODE_3D_DT64 | MODE_DC_DT64
        fr.mode = (gt_mode_d | empty_part[part_d] * dt64).to(torch.int32).contiguous()
        _, _, res = _run_stages(fr, self.plan, True)
        stat = torch.cat([b[6] for b in self.batches]).max().view(1) if self.batches else empty(torch.int32, 1)
        n_det = fr.dt_count.sum().view(1).to(torch.int64) if self.batches else empty(torch.int64, 1)
        h = torch.cat([res, stat.to(torch.int64), n_det]).cpu().numpy()        # the one read
        if int(h[-2]):
            raise RuntimeError("KITTI prediction conversion: frame index out of range")
        compute_aos = bool(h[-1] > 0)
        return compose(self.plan.layout.host_views(h[:-2]), self.plan, compute_aos, PR_detail_dict)
