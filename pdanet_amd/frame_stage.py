"""Preparing frames on the device: KITTI's field-of-view filter and the gt_sampling database.

fov_filter is KittiDataset's FOV_POINTS_ONLY step (pcdet/datasets/kitti/kitti_dataset.py:407-413: calib.lidar_to_rect,
calib.rect_to_img, get_fov_flag) for a batch of raw scans.  It produces the packed (points, offsets, n_cap) form that
DataAugmentor.__call__ and DataProcessor.__call__ take, so a raw scan reaches the detector without leaving the device.

GtDatabaseBuilder is create_groundtruth_database (kitti_dataset.py:224-274, once_dataset.py:300-350) for batches of
frames: the points inside every annotated box (the CPU test points_in_boxes_cpu), relative to the box centre.  It can
hand the result straight to the augmentor (finish -> GtDatabase, the points never leave the device) or write the
reference's files (write -> gt_database/*.bin and the dbinfos pickle, which GtDatabase.from_dbinfos and the reference
read alike).

Both run in csrc/frame_stage.hip (include/pda_train.h pda_kitti_fov_filter, pda_gt_extract_count / _write).  Reading label,
calibration and plane files stays with the caller.
"""
import os
import pickle

import numpy as np
import torch

from .data_augmentor import GtDatabase, _filter_by_min_points
from .pointnet2_batch_cuda import F32, _call, _chk
from .stage_common import (STATUS_BAD_OFFSETS, STATUS_OVER_CAP, cfg_get, current_device, offsets_of, pack_scenes, packed_form,
                           raise_on_status, upload, workspace)

MAX_BOXES_PER_FRAME = 256
# info[:, 3] status bits (include/pda_train.h) next to the two shared ones, and what check=True raises for each
STATUS_OVER_BOXES = 8
_RULES = [(STATUS_BAD_OFFSETS, ": offsets outside the packed points or boxes"),
          (STATUS_OVER_CAP, ": more than n_cap points or an output capacity exceeded"),
          (STATUS_OVER_BOXES, ": more than %d boxes" % MAX_BOXES_PER_FRAME)]
CALIB_RECORD_FLOATS = 24
KITTI_KEYS = ('name', 'path', 'image_idx', 'gt_idx', 'box3d_lidar', 'num_points_in_gt', 'difficulty', 'bbox', 'score')
ONCE_KEYS = ('name', 'path', 'gt_idx', 'box3d_lidar', 'num_points_in_gt')


def calib_records(calibs):
    """(n, 24) float32 rows M | P2 for pda_kitti_fov_filter, from Calibration objects, their dicts or the (n, 33) rows
    P2 | R0 | V2C of kitti_eval.calib_matrix.  M = np.dot(V2C.T, R0.T) in float32, as Calibration.lidar_to_rect forms it."""
    from .kitti_eval import CALIB_FLOATS, calib_matrix
    rows = calibs if isinstance(calibs, np.ndarray) else calib_matrix(list(calibs))
    rows = np.asarray(rows, np.float32).reshape(-1, CALIB_FLOATS)
    out = np.zeros((rows.shape[0], CALIB_RECORD_FLOATS), np.float32)
    for i, r in enumerate(rows):
        p2, r0, v2c = r[:12].reshape(3, 4), r[12:21].reshape(3, 3), r[21:33].reshape(3, 4)
        out[i, :12] = np.dot(v2c.T, r0.T).reshape(12)
        out[i, 12:] = p2.reshape(12)
    return out


def fov_filter(points, calibs, image_shapes, check=True):
    """points: a list of B (n_i, C) host arrays, or a tuple (packed (n_total, C) float32, offsets (B + 1) int64, n_cap)
    of device tensors.  calibs: per scene a Calibration (or its dict), the (B, 33) rows of kitti_eval.calib_matrix, or a
    device tensor (B, 24) made from calib_records.  image_shapes: (B, 2) (H, W), host or an int32 device tensor.
    check: read info once and raise ValueError on a status bit (offsets outside the buffer, more than n_cap rows).  With
    device points and check=False nothing is read back.
    Returns ((packed (rows, C), offsets (B + 1), n_cap), info (B, 4) int32 [n_in, n_kept, 0, status]): the kept rows of
    every scene in their order; the first part feeds DataAugmentor.__call__ / DataProcessor.__call__ unchanged."""
    dev_in = isinstance(points, tuple)
    if dev_in:
        pts, offs, n_cap = packed_form(points)
        dev, host = pts.device, []
    else:
        packed, offs, n_cap, _ = pack_scenes(points)
        dev, host = current_device(), [offs, packed]
    B = offs.shape[0] - 1
    cal_dev = isinstance(calibs, torch.Tensor)
    if not cal_dev:
        host.append(calib_records(calibs))
        if host[-1].shape[0] != B:
            raise ValueError("calibs needs one entry per scene")
    shp_dev = isinstance(image_shapes, torch.Tensor) and image_shapes.is_cuda
    if not shp_dev:
        host.append(np.asarray(image_shapes.cpu() if isinstance(image_shapes, torch.Tensor) else image_shapes).astype(np.int32).reshape(-1, 2))
        if host[-1].shape[0] != B:
            raise ValueError("image_shapes needs one (H, W) per scene")
    views = iter(upload(host, dev, pinned=True)) if host else iter(())
    if not dev_in:
        offs, pts = next(views), next(views)
    cal = calibs if cal_dev else next(views)
    shp = image_shapes if shp_dev else next(views)
    if cal.shape != (B, CALIB_RECORD_FLOATS) or shp.shape != (B, 2):
        raise ValueError("calibs must be (B, 24) and image_shapes (B, 2)")
    n_total, C = pts.shape
    if C < 3:
        raise ValueError("points need at least x, y, z")
    ws = workspace("pda_kitti_fov_filter_workspace_bytes", (B, n_cap), "batch %d / n_cap %d out of range" % (B, n_cap), dev)
    out = torch.empty((max(n_total, 1), C), dtype=torch.float32, device=dev)
    out_offs = torch.empty((B + 1,), dtype=torch.int64, device=dev)
    info = torch.empty((B, 4), dtype=torch.int32, device=dev)
    _call("pda_kitti_fov_filter", pts, _chk(pts, "points", F32) if n_total else None, _chk(offs, "offsets", torch.int64), n_total, B,
          C, n_cap, _chk(cal, "calibs", F32), _chk(shp, "image_shapes", torch.int32), out.data_ptr(), n_total,
          out_offs.data_ptr(), info.data_ptr(), ws.data_ptr())
    if check:
        raise_on_status(info.cpu(), _RULES)
    return (out, out_offs, n_cap), info


def gt_extract(points, boxes, box_offsets, centre, check=True):
    """The points inside every box of its own frame, relative to the box centre (pda_gt_extract_count / _write).
    points: (packed (n_total, C) float32, offsets (B + 1) int64, n_cap) on the device; boxes (m_total, 7) float32,
    box_offsets (B + 1) int64, centre (m_total, 3) float64, all on the device.  The total is read once between the two
    entries.  Returns (obj_points (rows, C), obj_offsets (m_total + 1) int64, counts (m_total) int32, info (B, 4))."""
    pts, offs, n_cap = points
    dev = pts.device
    B, n_total, C, m_total, n_cap = offs.numel() - 1, pts.shape[0], pts.shape[1], boxes.shape[0], int(n_cap)
    if boxes.dim() != 2 or boxes.shape[1] != 7 or tuple(centre.shape) != (m_total, 3):
        raise ValueError("boxes must be (m_total, 7) and centre (m_total, 3)")
    ws = workspace("pda_gt_extract_workspace_bytes", (B, n_cap, m_total),
                   "batch %d / n_cap %d / %d boxes out of range" % (B, n_cap, m_total), dev)
    counts = torch.empty((m_total,), dtype=torch.int32, device=dev)
    info = torch.empty((B, 4), dtype=torch.int32, device=dev)
    head = (_chk(pts, "points", F32) if n_total else None, _chk(offs, "offsets", torch.int64), n_total, B, C, n_cap,
            _chk(boxes, "boxes", F32) if m_total else None, _chk(box_offsets, "box_offsets", torch.int64), m_total)
    _call("pda_gt_extract_count", pts, *head, counts.data_ptr() if m_total else None, info.data_ptr(), ws.data_ptr())
    obj_offs = torch.zeros((m_total + 1,), dtype=torch.int64, device=dev)
    obj_offs[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
    total = int(obj_offs[-1].item())                     # the one host read: sizes the output
    obj_points = torch.empty((max(total, 1), C), dtype=torch.float32, device=dev)
    _call("pda_gt_extract_write", pts, *head, _chk(centre, "centre", torch.float64) if m_total else None, obj_offs.data_ptr(),
          obj_points.data_ptr(), total, info.data_ptr(), ws.data_ptr())
    if check:
        raise_on_status(info.cpu(), _RULES, "frame")
    return obj_points[:total], obj_offs, counts, info


def _difficulty_filter(db_infos, removed):
    return {k: [i for i in v if i['difficulty'] not in removed] for k, v in db_infos.items()}


class GtDatabaseBuilder:
    """create_groundtruth_database for batches of frames.  used_classes: the reference's argument (KITTI: only these
    classes get an info entry, every object still gets its .bin file; None = every class)."""

    def __init__(self, used_classes=None, num_point_features=4):
        self.used_classes = None if used_classes is None else list(used_classes)
        self.num_point_features = int(num_point_features)
        self.objects = []        # one record per object, in frame and box order
        self._batches = []       # (obj_points (rows, C) device, first object id, obj_offsets host)
        self._rows = 0

    # ---- filling ---------------------------------------------------------------------------------------------------------
    def add_counted(self, frame_id, names, gt_boxes, counts, extra=None):
        """Register the objects of one frame whose point counts are known (host only; add_frames calls this)."""
        gt_boxes = np.asarray(gt_boxes)
        gt_boxes = gt_boxes.reshape(len(names), -1) if len(names) else np.zeros((0, 7), gt_boxes.dtype)
        if gt_boxes.shape[0] and gt_boxes.shape[1] != 7:
            raise NotImplementedError("boxes with %d values: boxes with velocities are not supported" % gt_boxes.shape[1])
        if len(counts) != len(names):
            raise ValueError("frame %s: %d names but %d counts" % (frame_id, len(names), len(counts)))
        extra = extra or {}
        for key, val in extra.items():
            if len(val) != len(names):
                raise ValueError("frame %s: extra[%r] needs one value per object" % (frame_id, key))
        for i, name in enumerate(names):
            self.objects.append({'frame_id': frame_id, 'name': name, 'gt_idx': i, 'box3d_lidar': gt_boxes[i],
                                 'num_points_in_gt': int(counts[i]), 'extra': {k: v[i] for k, v in extra.items()}})

    def add_frames(self, points, gt_boxes, names, frame_ids, extra=None):
        """points: a list of B (n_i, C) host arrays or a device tuple (packed, offsets, n_cap); gt_boxes: per frame the
        (m_i, 7) lidar boxes as the infos hold them (float64 for KITTI's gt_boxes_lidar and ONCE's boxes_3d); names: per
        frame the object names; frame_ids: per frame what the file names start with (KITTI's lidar_idx, ONCE's frame_id);
        extra: {key: per frame, one value per object} passed through to the infos (KITTI: difficulty, bbox, score,
        image_idx)."""
        B = len(frame_ids)
        if len(gt_boxes) != B or len(names) != B:
            raise ValueError("gt_boxes, names and frame_ids need one entry per frame")
        if isinstance(points, tuple):
            pts, offs, n_cap = points
            dev = pts.device
        else:
            if len(points) != B:
                raise ValueError("points needs one entry per frame")
            packed, offs_h, n_cap, _ = pack_scenes(points)
            dev = current_device()
            pts, offs = torch.from_numpy(packed).to(dev), torch.from_numpy(offs_h).to(dev)
        if pts.shape[1] != self.num_point_features:
            raise ValueError("the builder holds %d point features, the frames %d" % (self.num_point_features, pts.shape[1]))
        rows = [np.asarray(g).reshape(len(nm), -1) if len(nm) else np.zeros((0, 7)) for g, nm in zip(gt_boxes, names)]
        if any(r.shape[1] != 7 for r in rows):
            raise NotImplementedError("boxes with more than 7 values (velocities) are not supported")
        allb = np.concatenate(rows, 0) if rows else np.zeros((0, 7))
        boffs = offsets_of([len(r) for r in rows])
        d_boxes = torch.from_numpy(np.ascontiguousarray(allb.astype(np.float32))).to(dev)
        d_centre = torch.from_numpy(np.ascontiguousarray(allb[:, :3].astype(np.float64))).to(dev)
        obj_points, obj_offs, counts, _ = gt_extract((pts, offs, n_cap), d_boxes, torch.from_numpy(boffs).to(dev), d_centre)
        counts_h = counts.cpu().numpy()
        first = len(self.objects)
        for b in range(B):
            s, e = int(boffs[b]), int(boffs[b + 1])
            self.add_counted(frame_ids[b], list(names[b]), rows[b], counts_h[s:e],
                             {k: v[b] for k, v in extra.items()} if extra else None)
        self._batches.append((obj_points, first, obj_offs.cpu().numpy()))
        self._rows += obj_points.shape[0]

    # ---- the infos ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def file_name(obj):
        return '%s_%s_%d.bin' % (obj['frame_id'], obj['name'], obj['gt_idx'])

    def dbinfos(self, dataset='kitti', split='train'):
        """all_db_infos as create_groundtruth_database pickles it: {name: [info]} in order of first appearance."""
        if dataset not in ('kitti', 'once'):
            raise ValueError("dataset must be 'kitti' or 'once'")
        folder = 'gt_database' if split == 'train' else 'gt_database_%s' % split
        out = {}
        for obj in self.objects:
            name = obj['name']
            if dataset == 'kitti' and self.used_classes is not None and name not in self.used_classes:
                continue
            info = {'name': name, 'path': folder + '/' + self.file_name(obj)}
            ex = obj['extra']
            if dataset == 'kitti':
                info['image_idx'] = ex.get('image_idx', obj['frame_id'])
            info.update(gt_idx=obj['gt_idx'], box3d_lidar=obj['box3d_lidar'], num_points_in_gt=obj['num_points_in_gt'])
            if dataset == 'kitti':
                for key in ('difficulty', 'bbox', 'score'):
                    if key not in ex:
                        raise ValueError("KITTI infos need extra[%r]" % key)
                    info[key] = ex[key]
            out.setdefault(name, []).append(info)
        return out

    def _device_points(self):
        if sum(len(o) - 1 for _, _, o in self._batches) != len(self.objects):
            raise ValueError("objects registered with add_counted have no points")
        offs = [np.zeros(1, np.int64)]
        at = 0
        for p, _, o in self._batches:
            offs.append(o[1:] + at)
            at += p.shape[0]
        if not self._batches:
            return torch.zeros((0, self.num_point_features), dtype=torch.float32, device=current_device()), offs[0]
        return torch.cat([p for p, _, _ in self._batches], 0), np.concatenate(offs)

    def finish(self, class_names, sampler_cfg=None):
        """The GtDatabase of CLASS_NAMES with sampler_cfg's PREPARE applied (filter_by_min_points, filter_by_difficulty)
        as GtDatabase.from_dbinfos applies it.  The points stay on the device."""
        db_infos = {name: [] for name in class_names}
        for o, obj in enumerate(self.objects):
            if obj['name'] in db_infos and (self.used_classes is None or obj['name'] in self.used_classes):
                db_infos[obj['name']].append(dict(obj, _id=o, **obj['extra']))
        for func, val in (cfg_get(sampler_cfg, 'PREPARE', {}) if sampler_cfg is not None else {}).items():
            if func == 'filter_by_min_points':
                db_infos = _filter_by_min_points(db_infos, val)
            elif func == 'filter_by_difficulty':
                db_infos = _difficulty_filter(db_infos, val)
            else:
                raise NotImplementedError("PREPARE step %r" % func)
        points, offsets = self._device_points()
        ids = [i['_id'] for name in class_names for i in db_infos[name]]
        boxes = {name: (np.stack([np.asarray(i['box3d_lidar'], np.float64) for i in db_infos[name]]) if db_infos[name]
                        else np.zeros((0, 7))) for name in class_names}
        return GtDatabase.from_device(class_names, boxes, points, offsets, ids)

    def write(self, root_path, dataset='kitti', split='train'):
        """gt_database/<frame>_<name>_<i>.bin for every object and kitti_dbinfos_<split>.pkl / once_dbinfos_<split>.pkl
        under root_path, as the reference lays them out.  Returns the path of the info file."""
        infos = self.dbinfos(dataset, split)
        folder = os.path.join(str(root_path), 'gt_database' if split == 'train' else 'gt_database_%s' % split)
        os.makedirs(folder, exist_ok=True)
        for p, first, o in self._batches:
            host = p.cpu().numpy()
            for k in range(len(o) - 1):
                host[o[k]:o[k + 1]].tofile(os.path.join(folder, self.file_name(self.objects[first + k])))
        path = os.path.join(str(root_path), '%s_dbinfos_%s.pkl' % (dataset, split))
        with open(path, 'wb') as f:
            pickle.dump(infos, f)
        return path
