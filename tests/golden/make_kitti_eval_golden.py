#!/usr/bin/env python
"""Generates tests/golden/kitti_eval.npz: the REFERENCE's KITTI evaluation
(pcdet/datasets/kitti/kitti_object_eval_python/eval.py, rotate_iou.py) run on ~30 synthetic KITTI-like frames, and its
generate_prediction_dicts geometry (pcdet/utils/calibration_kitti.py, box_utils.py) on a few synthetic calibrations.

numba is stubbed (reference_loader.stub_numba), and rotate_iou_gpu_eval is a loop over the reference's own
devRotateIoUEval(query_k, box_n, criterion) with the same float32 casts and return dtype.  clean_data, get_thresholds and fused_compute_statistics are wrapped to record the
flags, num_valid_gt, thresholds and pr table of every (metric, class, difficulty, overlap setting); the per-frame
overlap blocks come from the reference's calculate_iou_partly(dt_annos, gt_annos, metric).

The scenes hold Car / Pedestrian / Cyclist / Van / Person_sitting / Truck / Misc / DontCare GT with occlusion 0-3,
truncation on and next to 0.15 / 0.3 / 0.5 and bbox heights next to 25 and 40; detections jittered from GT, shorter than
the minimum height, false positives under DontCare boxes, exact score ties, a frame without detections, a frame without
GT, a class without valid GT (Truck) and one frame with more than 64 GT and 256 detections.  Knife edges are redrawn:
|overlap - thr| < 1e-3 for 0.25 / 0.5 / 0.7 in every metric (DontCare overlaps included) and heights within 1e-3 of
25 / 40.  Config 'aos' has real alphas; config 'no_aos' the same detections with alpha = -10 and the empty frame in the
float64 template of generate_prediction_dicts.

Run with the reference checkout:  python tests/golden/make_kitti_eval_golden.py /path/to/reference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from reference_loader import extension_stubs, load, reference_root, stub_numba  # noqa: E402

NAMES = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'Truck', 'Misc', 'DontCare']
CLASSES = ['Car', 'Pedestrian', 'Cyclist', 'Truck']
DIMS = {'Car': (3.9, 1.55, 1.6), 'Pedestrian': (0.8, 1.75, 0.6), 'Cyclist': (1.75, 1.7, 0.6), 'Van': (5.0, 2.1, 1.9),
        'Person_sitting': (0.8, 1.2, 0.6), 'Truck': (10.0, 3.2, 2.6), 'Misc': (3.0, 1.8, 1.5),
        'DontCare': (-1.0, -1.0, -1.0)}
THRS = (0.25, 0.5, 0.7)
IMG_W, IMG_H = 1242, 375


ROT = EV = BOX = CAL = None      # the reference's rotate_iou, eval, box_utils and calibration_kitti, once load_reference has run


def load_reference(root):
    global ROT, EV, BOX, CAL
    stub_numba()
    kitti_eval = "datasets.kitti.kitti_object_eval_python."
    # box_utils without common_utils and the compiled ops, which it imports but these functions do not use
    ROT, EV, BOX, CAL = load(root, "pcdet_ref", [kitti_eval + "rotate_iou", kitti_eval + "eval", "utils.box_utils",
                                                 "utils.calibration_kitti"], stubs=extension_stubs({"utils.common_utils": {}}))
    EV.rotate_iou_gpu_eval = rotate_iou_loop


def rotate_iou_loop(boxes, query_boxes, criterion=-1, device_id=0):
    """rotate_iou_gpu_eval with its kernel body called per pair: dev_iou[n, k] = devRotateIoUEval(query_k, box_n)."""
    b32, q32 = boxes.astype(np.float32), query_boxes.astype(np.float32)
    iou = np.zeros((b32.shape[0], q32.shape[0]), np.float32)
    for n in range(b32.shape[0]):
        for k in range(q32.shape[0]):
            iou[n, k] = ROT.devRotateIoUEval(np.ascontiguousarray(q32[k]), np.ascontiguousarray(b32[n]), criterion)
    return iou.astype(b32.dtype)


# ---- scenes ------------------------------------------------------------------------------------------------------------
def _rot_y_box(loc, dims, ry):
    """Camera box -> its 8 corners (for a plausible image box)."""
    l, h, w = dims
    xs = np.array([l, l, -l, -l, l, l, -l, -l]) / 2
    zs = np.array([w, -w, -w, w, w, -w, -w, w]) / 2
    ys = np.array([0, 0, 0, 0, -h, -h, -h, -h])
    c, s = np.cos(ry), np.sin(ry)
    return np.stack([loc[0] + xs * c + zs * s, loc[1] + ys, loc[2] - xs * s + zs * c], 1)


def _image_box(loc, dims, ry):
    pts = _rot_y_box(loc, dims, ry)
    f = 720.0
    u = f * pts[:, 0] / pts[:, 2] + IMG_W / 2
    v = f * pts[:, 1] / pts[:, 2] + IMG_H / 2
    return np.array([max(u.min(), 0), max(v.min(), 0), min(u.max(), IMG_W - 1), min(v.max(), IMG_H - 1)])


def _height_ok(b):
    h = float(np.float32(b[3]) - np.float32(b[1]))
    return abs(h - 25) >= 1e-3 and abs(h - 40) >= 1e-3


def _gt_object(rng, name):
    while True:
        if name == 'DontCare':
            x0, y0 = rng.uniform(0, IMG_W - 120), rng.uniform(120, 260)
            bbox = np.array([x0, y0, x0 + rng.uniform(20, 120), y0 + rng.uniform(15, 60)])
            return dict(name=name, bbox=bbox, loc=np.array([-1000.0, -1000, -1000]), dims=np.array([-1.0, -1, -1]),
                        ry=-10.0, alpha=-10.0, trunc=-1.0, occ=-1.0)
        dims = np.array(DIMS[name]) * rng.uniform(0.9, 1.1, 3)
        z = rng.uniform(6, 45)
        loc = np.array([rng.uniform(-0.6, 0.6) * z, rng.uniform(1.4, 1.9), z])
        ry = rng.uniform(-np.pi, np.pi)
        bbox = _image_box(loc, dims, ry)
        if bbox[2] - bbox[0] < 4 or not _height_ok(bbox):
            continue
        trunc = float(rng.choice([0.0, 0.0, 0.15, 0.3, 0.5, 0.14, 0.31, 0.49, 0.51, 0.16, 0.29, 0.7]))
        return dict(name=name, bbox=bbox, loc=loc, dims=dims, ry=ry, alpha=ry - np.arctan2(loc[0], loc[2]),
                    trunc=trunc, occ=float(rng.integers(0, 4)))


def _gt_anno(objs):
    n = len(objs)
    g = lambda k: [o[k] for o in objs]
    return {'name': np.array(g('name'), dtype='<U14').reshape(n),
            'truncated': np.array(g('trunc'), np.float64).reshape(n),
            'occluded': np.array(g('occ'), np.float64).reshape(n),
            'alpha': np.array(g('alpha'), np.float64).reshape(n),
            'bbox': np.array(g('bbox'), np.float32).reshape(n, 4),
            'dimensions': np.array(g('dims'), np.float64).reshape(n, 3),
            'location': np.array(g('loc'), np.float32).reshape(n, 3),
            'rotation_y': np.array(g('ry'), np.float64).reshape(n)}


def _dt_anno(dets, f64_empty=False):
    n = len(dets)
    if n == 0:
        dt = np.float64 if f64_empty else np.float32
        return {'name': np.zeros(0), 'truncated': np.zeros(0), 'occluded': np.zeros(0), 'alpha': np.zeros(0, dt),
                'bbox': np.zeros([0, 4], dt), 'dimensions': np.zeros([0, 3], dt), 'location': np.zeros([0, 3], dt),
                'rotation_y': np.zeros(0, dt), 'score': np.zeros(0, dt)}
    g = lambda k: [d[k] for d in dets]
    return {'name': np.array(g('name')), 'truncated': np.zeros(n), 'occluded': np.zeros(n),
            'alpha': np.array(g('alpha'), np.float32), 'bbox': np.array(g('bbox'), np.float32).reshape(n, 4),
            'dimensions': np.array(g('dims'), np.float32).reshape(n, 3),
            'location': np.array(g('loc'), np.float32).reshape(n, 3),
            'rotation_y': np.array(g('ry'), np.float32), 'score': np.array(g('score'), np.float32)}


def _overlaps_ok(gt, d):
    """Every metric's overlap of the detection with every GT, and its DontCare overlaps, away from the thresholds."""
    da = _dt_anno([dict(d, score=np.float32(0.5))])
    g = gt
    if len(g['name']) == 0:
        return True
    for metric in range(3):
        try:
            ov = EV.calculate_iou_partly([da], [g], metric, 1)[0][0].astype(np.float64)
        except IndexError:             # the stubbed point buffer overflowed (coincident edges)
            return False
        if not np.isfinite(ov).all() or np.abs(ov.reshape(-1, 1) - np.array(THRS)).min() < 1e-3:
            return False
    dc = g['bbox'][g['name'] == 'DontCare'].astype(np.float64)
    if len(dc):
        ov = EV.image_box_overlap(da['bbox'].astype(np.float64), dc, 0)
        if np.abs(ov.reshape(-1, 1) - np.array(THRS)).min() < 1e-3:
            return False
    return True


def _det_from(rng, o, name):
    for _ in range(100):
        loc = o['loc'] + np.r_[rng.normal(0, 0.15), rng.normal(0, 0.05), rng.normal(0, 0.2)]
        dims = o['dims'] * rng.uniform(0.92, 1.08, 3)
        ry = o['ry'] + rng.normal(0, 0.15)
        bbox = o['bbox'] + rng.normal(0, 4, 4)
        if bbox[3] - bbox[1] > 2 and _height_ok(bbox):
            return dict(name=name, bbox=bbox, loc=loc, dims=dims, ry=ry, alpha=o['alpha'] + rng.normal(0, 0.3))
    return None


def _det_free(rng, name, near=None):
    o = _gt_object(rng, name if name != 'DontCare' else 'Car')
    if near is not None:                   # a false positive under a DontCare box
        x0, y0, x1, y1 = near
        w, h = (x1 - x0) * rng.uniform(0.6, 1.0), (y1 - y0) * rng.uniform(0.6, 1.0)
        cx, cy = rng.uniform(x0 + w / 2, x1 - w / 2), rng.uniform(y0 + h / 2, y1 - h / 2)
        o['bbox'] = np.array([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
    return dict(name=name, bbox=o['bbox'], loc=o['loc'], dims=o['dims'], ry=o['ry'], alpha=o['alpha'])


def make_frame(rng, n_gt, n_fp, no_det=False):
    pool = ['Car'] * 5 + ['Pedestrian'] * 3 + ['Cyclist'] * 2 + ['Van', 'Person_sitting', 'Misc', 'DontCare', 'DontCare']
    objs = [_gt_object(rng, str(rng.choice(pool))) for _ in range(n_gt)]
    gt = _gt_anno(objs)
    if no_det:
        return gt, []
    dets = []
    ties = [0.5, 0.8, 0.3]
    for o in objs:
        if o['name'] == 'DontCare':
            if rng.random() < 0.7:
                cand = _det_free(rng, str(rng.choice(['Car', 'Pedestrian', 'Cyclist'])), near=o['bbox'])
            else:
                continue
        else:
            if rng.random() < 0.2:
                continue
            name = o['name'] if rng.random() < 0.85 else str(rng.choice(['Car', 'Pedestrian', 'Cyclist', 'Truck']))
            cand = _det_from(rng, o, name)
        for _ in range(2 if rng.random() < 0.1 else 1):
            if cand is not None:
                dets.append(cand)
    for _ in range(n_fp):
        dets.append(_det_free(rng, str(rng.choice(['Car', 'Pedestrian', 'Cyclist', 'Truck']))))
    out = []
    for d in dets:
        for _ in range(60):
            if _overlaps_ok(gt, d):
                break
            d = dict(d, loc=d['loc'] + rng.normal(0, 0.1, 3), bbox=d['bbox'] + rng.normal(0, 1.5, 4))
            if not (d['bbox'][3] - d['bbox'][1] > 2 and _height_ok(d['bbox'])):
                d['bbox'] = d['bbox'] + np.array([0, 0, 0, 1.0])
        else:
            continue
        s = float(rng.choice(ties)) if rng.random() < 0.2 else rng.uniform(0.05, 1.0)
        if out and rng.random() < 0.1:
            s = out[-1]['score']                              # exact tie with the previous detection
        out.append(dict(d, score=np.float32(s)))
    order = rng.permutation(len(out))
    return gt, [out[i] for i in order]


def build_scenes(seed=11):
    rng = np.random.default_rng(seed)
    frames = []
    for f in range(30):
        if f == 4:
            frames.append(make_frame(rng, 10, 3, no_det=True))
        elif f == 11:
            frames.append(make_frame(rng, 0, 6))
        elif f == 19:
            frames.append(make_frame(rng, 68, 250))
        else:
            frames.append(make_frame(rng, int(rng.integers(2, 16)), int(rng.integers(0, 8))))
    return frames


# ---- reference runs ------------------------------------------------------------------------------------------------------
def run_reference(gt_annos, dt_annos):
    rec = {'flags': [], 'thr': [], 'pr': []}
    orig_prep, orig_thr, orig_fused = EV._prepare_data, EV.get_thresholds, EV.fused_compute_statistics

    def prepare(gt, dt, current_class, difficulty):
        r = orig_prep(gt, dt, current_class, difficulty)
        rec['flags'].append((np.concatenate(r[2]) if r[2] else np.zeros(0, np.int64),
                             np.concatenate(r[3]) if r[3] else np.zeros(0, np.int64), int(r[6])))
        return r

    def thresholds(scores, num_gt, num_sample_pts=41):
        th = orig_thr(scores, num_gt, num_sample_pts)
        rec['thr'].append(list(th))
        return th

    def fused(overlaps, pr, *a, **k):
        orig_fused(overlaps, pr, *a, **k)
        rec['pr'].append(pr.copy())

    EV._prepare_data, EV.get_thresholds, EV.fused_compute_statistics = prepare, thresholds, fused
    try:
        detail = {}
        result, ret_dict = EV.get_official_eval_result([dict(a) for a in gt_annos], [dict(a) for a in dt_annos],
                                                       list(CLASSES), PR_detail_dict=detail)
    finally:
        EV._prepare_data, EV.get_thresholds, EV.fused_compute_statistics = orig_prep, orig_thr, orig_fused
    return result, ret_dict, detail, rec


def reference_overlaps(gt_annos, dt_annos):
    """Per metric, the frames' (GT x detection) blocks flattened, transposed from calculate_iou_partly(dt, gt)."""
    out = []
    for metric in range(3):
        blocks = EV.calculate_iou_partly(dt_annos, gt_annos, metric, len(gt_annos))[0]
        out.append(np.concatenate([b.astype(np.float64).T.reshape(-1) for b in blocks]))
    return np.stack(out)


def prediction_cases(rng, n_frames=4):
    """Synthetic calibrations and lidar boxes through the reference's generate_prediction_dicts geometry."""
    out = {'pred/boxes': [], 'pred/frame': [], 'pred/calib': [], 'pred/image_shape': []}
    res = {'pred/cam': [], 'pred/bbox': [], 'pred/alpha': []}
    for f in range(n_frames):
        a = rng.normal(0, 0.01, 3)
        Rz = np.array([[np.cos(a[0]), -np.sin(a[0]), 0], [np.sin(a[0]), np.cos(a[0]), 0], [0, 0, 1]])
        v2c_r = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]]) @ Rz
        V2C = np.c_[v2c_r, rng.normal([0, -0.08, -0.27], 0.02)].astype(np.float32)
        R0 = (np.eye(3) + rng.normal(0, 0.005, (3, 3))).astype(np.float32)
        fu = rng.uniform(700, 730)
        P2 = np.array([[fu, 0, rng.uniform(600, 620), rng.normal(45, 2)], [0, fu, rng.uniform(170, 180), rng.normal(0, 0.3)],
                       [0, 0, 1, rng.normal(0.003, 0.001)]], np.float32)
        calib = CAL.Calibration({'P2': P2, 'R0': R0, 'Tr_velo2cam': V2C})
        shape = np.array([IMG_H + f, IMG_W - 2 * f], np.int32)
        n = int(rng.integers(5, 12))
        boxes = np.c_[rng.uniform(3, 60, n), rng.uniform(-15, 15, n), rng.uniform(-2, 0, n),
                      rng.uniform(0.5, 5, n), rng.uniform(0.5, 2.5, n), rng.uniform(1.2, 2.2, n),
                      rng.uniform(-np.pi, np.pi, n)].astype(np.float32)
        cam = BOX.boxes3d_lidar_to_kitti_camera(boxes, calib)
        img = BOX.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=shape)
        alpha = -np.arctan2(-boxes[:, 1], boxes[:, 0]) + cam[:, 6]
        out['pred/boxes'].append(boxes)
        out['pred/frame'].append(np.full(n, f, np.int32))
        out['pred/calib'].append(np.concatenate([P2.reshape(-1), R0.reshape(-1), V2C.reshape(-1)]))
        out['pred/image_shape'].append(shape)
        res['pred/cam'].append(cam)
        res['pred/bbox'].append(img)
        res['pred/alpha'].append(alpha)
    d = {k: (np.concatenate(v) if k in ('pred/boxes', 'pred/frame') else np.stack(v)) for k, v in out.items()}
    d.update({k: np.concatenate(v) for k, v in res.items()})
    assert all(v.dtype in (np.float32, np.int32) for v in d.values())
    return d


def pack(frames, prefix, aos, out):
    gt_annos = [g for g, _ in frames]
    dt_annos = []
    for _, dets in frames:
        a = _dt_anno(dets, f64_empty=not aos)
        if not aos and len(dets):
            a['alpha'] = np.full(len(dets), -10, np.float32)
        dt_annos.append(a)
    result, ret_dict, detail, rec = run_reference(gt_annos, dt_annos)
    out[prefix + 'overlaps'] = reference_overlaps(gt_annos, dt_annos)
    C = len(CLASSES)
    flags = rec['flags'][:3 * C]                                   # the same for every metric
    out[prefix + 'gt_flags'] = np.stack([f[0] for f in flags]).astype(np.int8)
    out[prefix + 'dt_flags'] = np.stack([f[1] for f in flags]).astype(np.int8)
    out[prefix + 'num_valid_gt'] = np.array([f[2] for f in flags], np.int64)
    T = len(rec['thr'])
    assert T == 18 * C and len(rec['pr']) == T
    thr = np.zeros((T, 41))
    nthr = np.zeros(T, np.int64)
    pr = np.zeros((T, 41, 4))
    for t in range(T):
        nthr[t] = len(rec['thr'][t])
        thr[t, :nthr[t]] = rec['thr'][t]
        pr[t, :nthr[t]] = rec['pr'][t]
    out[prefix + 'thresholds'], out[prefix + 'n_thresholds'], out[prefix + 'pr'] = thr, nthr, pr
    out[prefix + 'result'] = np.array(result)
    out[prefix + 'keys'] = np.array(list(ret_dict))
    out[prefix + 'values'] = np.array([float(v) for v in ret_dict.values()], np.float64)
    for k, v in detail.items():
        out[prefix + 'detail/' + k] = v
    print(prefix, result)
    return gt_annos, dt_annos


def main():
    load_reference(reference_root())
    frames = build_scenes()
    out = {'names': np.array(NAMES), 'classes': np.array(CLASSES)}
    gt_annos, dt_annos = pack(frames, 'aos/', True, out)
    pack(frames, 'no_aos/', False, out)
    ng = np.array([len(a['name']) for a in gt_annos])
    nd = np.array([len(a['name']) for a in dt_annos])
    print("frames %d, GT %d, detections %d, largest frame %d x %d" % (len(ng), ng.sum(), nd.sum(), ng.max(), nd.max()))
    width = {'bbox': 4, 'location': 3, 'dimensions': 3}
    cat = lambda annos, k, dt: np.concatenate([np.asarray(a[k], dt).reshape(len(a['name']), width.get(k, 1))
                                               for a in annos])
    out.update({'gt_count': ng.astype(np.int64), 'gt_name': np.concatenate([[NAMES.index(n) for n in a['name']]
                                                                          for a in gt_annos]).astype(np.int32),
                'gt_bbox': cat(gt_annos, 'bbox', np.float32), 'gt_location': cat(gt_annos, 'location', np.float32),
                'gt_dimensions': cat(gt_annos, 'dimensions', np.float64),
                'gt_rotation_y': cat(gt_annos, 'rotation_y', np.float64)[:, 0],
                'gt_alpha': cat(gt_annos, 'alpha', np.float64)[:, 0],
                'gt_truncated': cat(gt_annos, 'truncated', np.float64)[:, 0],
                'gt_occluded': cat(gt_annos, 'occluded', np.float64)[:, 0],
                'dt_count': nd.astype(np.int64), 'dt_name': np.concatenate([[NAMES.index(str(n)) for n in a['name']]
                                                                           for a in dt_annos]).astype(np.int32),
                'dt_bbox': cat(dt_annos, 'bbox', np.float32), 'dt_location': cat(dt_annos, 'location', np.float32),
                'dt_dimensions': cat(dt_annos, 'dimensions', np.float32),
                'dt_rotation_y': cat(dt_annos, 'rotation_y', np.float32)[:, 0],
                'dt_alpha': cat(dt_annos, 'alpha', np.float32)[:, 0], 'dt_score': cat(dt_annos, 'score', np.float32)[:, 0]})
    out.update(prediction_cases(np.random.default_rng(3)))
    path = os.path.join(HERE, "kitti_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
