"""The input stage of the data loader on the device: ragged raw scenes -> the collated batch detector.IASSD takes.

The reference prepares every scene on the host in numpy (pcdet/datasets/processor/data_processor.py:
mask_points_and_boxes_outside_range -> sample_points -> shuffle_points) and collates the batch afterwards
(pcdet/datasets/dataset.py DatasetTemplate.collate_batch).  DataProcessor reads the same DATA_PROCESSOR list and runs the
whole chain for all scenes of a batch in five launches (csrc/input_stage.hip, include/pda_train.h pda_input_stage /
pda_input_boxes).

Randomness: with `draws` the caller passes the draws the reference would make (explicit mode, index-exact); otherwise
they are generated on the device from a 64-bit `seed` (seeded mode), which is drawn from torch's CPU generator when not
given, so torch.manual_seed makes a run reproducible.  Seeded mode approximates the reference's distribution (uniform
samples without replacement, uniform shuffles, uniform draws with replacement) with keyed Feistel bijections and a counter
hash -- tested statistically, not exactly uniform -- and does not reproduce numpy's stream.

Boxes are padded to a fixed capacity `max_gt`: the head's graphs (detector.IASSD graph_head / graph_tail) key on argument
shapes, and the reference's "largest count in the batch" would change the shape, and capture a new graph, from batch to
batch.  With max_gt given and check=False the call reads nothing back and can be captured into a graph; scenes the
reference would reject are then only flagged in batch_dict['input_info'] (see DataProcessor.__call__).
"""
import ctypes

import numpy as np
import torch

from .pointnet2_batch_cuda import F32, _call, _chk
from .stage_common import (STATUS_BAD_OFFSETS, STATUS_OVER_CAP, cfg_get, current_device, offsets_of, pack_scenes, packed_form,
                           raise_on_status, upload, workspace)
from .voxel_utils import VoxelSpec

# input_info[:, 3] status bits (include/pda_train.h pda_input_stage) next to the two shared ones; voxel_info[:, 3] adds
# STATUS_VOXEL_CAP (pda_voxel_sample)
STATUS_EMPTY, STATUS_BAD_DRAW, STATUS_VOXEL_CAP = 1, 8, 16
_BAD_SCENE = (STATUS_BAD_OFFSETS | STATUS_OVER_CAP, ": offsets outside the packed points or more than n_cap points")
_INPUT_RULES = [_BAD_SCENE, (STATUS_EMPTY, " has no point inside POINT_CLOUD_RANGE"), (STATUS_BAD_DRAW, ": a draw is out of range")]
_VOXEL_RULES = [_BAD_SCENE, (STATUS_BAD_DRAW, ": perm0 is not a permutation of the masked points")]
_STEPS = ("mask_points_and_boxes_outside_range", "sample_points", "shuffle_points")
_VOXEL_STEPS = ("mask_points_and_boxes_outside_range", "shuffle_points", "sample_points_by_voxels")


class DataProcessor:
    """DATA_PROCESSOR of a reference-shaped yaml: mask_points_and_boxes_outside_range, sample_points and shuffle_points,
    in this order (each optional except sample_points), or mask_points_and_boxes_outside_range, shuffle_points and
    sample_points_by_voxels in this order (each optional except the last).  Anything else raises NotImplementedError."""

    def __init__(self, processor_cfg, point_cloud_range, training, num_point_features):
        self.point_cloud_range = np.asarray(point_cloud_range, dtype=np.float32)
        if self.point_cloud_range.shape != (6,):
            raise ValueError("point_cloud_range must hold 6 values")
        self.training = bool(training)
        self.mode = 'train' if self.training else 'test'
        self.num_point_features = int(num_point_features)
        self.mask_points, self.remove_outside_boxes, self.min_num_corners = False, False, 1
        self.num_points, self.shuffle = None, False
        self.voxel, self.sample_type, self.shuffle_first = None, None, False
        for cfg in processor_cfg:
            if cfg['NAME'] not in _STEPS + _VOXEL_STEPS:
                raise NotImplementedError("DATA_PROCESSOR step %r has no device implementation" % cfg['NAME'])
        steps = _VOXEL_STEPS if any(cfg['NAME'] == 'sample_points_by_voxels' for cfg in processor_cfg) else _STEPS
        last = -1
        for cfg in processor_cfg:
            name = cfg['NAME']
            if name not in steps or steps.index(name) <= last:
                raise NotImplementedError("DATA_PROCESSOR steps must come in the order %s" % (steps,))
            last = steps.index(name)
            if name == 'mask_points_and_boxes_outside_range':
                self.mask_points = True
                self.remove_outside_boxes = bool(cfg_get(cfg, 'REMOVE_OUTSIDE_BOXES', False)) and self.training
                self.min_num_corners = int(cfg_get(cfg, 'min_num_corners', 1))
            elif name == 'sample_points':
                self.num_points = int(cfg['NUM_POINTS'][self.mode])
                if self.num_points == -1:
                    raise ValueError("sample_points NUM_POINTS == -1 keeps ragged scenes: the backbone needs the same "
                                     "number of points in every scene")
                if self.num_points < 1:
                    raise ValueError("sample_points NUM_POINTS must be positive")
            elif name == 'sample_points_by_voxels':
                self.num_points = int(cfg['NUM_POINTS'][self.mode])
                if self.num_points == -1:
                    raise ValueError("sample_points_by_voxels NUM_POINTS == -1 (dynamic voxelization) keeps ragged scenes: the "
                                     "backbone needs the same number of points in every scene")
                if self.num_points < 1:
                    raise ValueError("sample_points_by_voxels NUM_POINTS must be positive")
                self.sample_type = str(cfg_get(cfg, 'SAMPLE_TYPE', 'raw'))
                if self.sample_type not in ('raw', 'mean_vfe'):
                    # the reference treats every other value as 'raw'; a typo should not pass silently
                    raise ValueError("sample_points_by_voxels SAMPLE_TYPE must be 'raw' or 'mean_vfe'")
                self.voxel = VoxelSpec(self.point_cloud_range, cfg['VOXEL_SIZE'], cfg['MAX_POINTS_PER_VOXEL'],
                                       cfg['MAX_NUMBER_OF_VOXELS'][self.mode])
            elif steps is _VOXEL_STEPS:
                self.shuffle_first = bool(cfg['SHUFFLE_ENABLED'][self.mode])
            else:
                self.shuffle = bool(cfg['SHUFFLE_ENABLED'][self.mode])
        if self.num_points is None:
            raise ValueError("DATA_PROCESSOR needs a sample_points step (the backbone needs equal scene sizes)")
        inf = np.float32(np.inf)
        # in the voxel chain the mask runs in the voxel stage, in front of the shuffle
        self._point_range = (self.point_cloud_range if self.mask_points and self.voxel is None
                             else np.array([-inf, -inf, -inf, inf, inf, inf], np.float32))
        self._range_c = (ctypes.c_float * 6)(*self._point_range.tolist())

    # ------------------------------------------------------------------------------------------------------------------
    def __call__(self, points, gt_boxes=None, max_gt=None, seed=None, draws=None, check=True, device=None):
        """points: a list of B (n_i, C) arrays (numpy / torch, host or device), or a tuple (packed (n_total, C) float32,
        offsets (B + 1) int64, n_cap) of device tensors with n_cap >= every n_i.
        gt_boxes: None, a list of B (m_i, box_dim) arrays, or a tuple (packed (m_total, box_dim), box_offsets (B + 1)
        int64) of device tensors.
        max_gt: the box capacity of batch_dict['gt_boxes'] (B, max_gt, box_dim); None pads to the largest kept count of
        the batch, as collate_batch does (that needs a host read).
        seed / draws: see the module docstring; draws = dict(pick=, perm1=, perm2=) with one int array per scene (or a
        (B, k) array): pick = the ranks sample_points draws (into the near list in case A, the masked list in case B,
        the extra draws in case C), perm1 = its shuffle, perm2 = shuffle_points' permutation (when it is enabled).  In the
        voxel chain the ranks refer to the voxel rows, and perm0 = the leading shuffle_points' permutation of the masked
        points (when it is enabled), one int array of that length per scene.
        check: read batch_dict['input_info'] once and raise ValueError on a scene with no point in range (the reference
        raises there), on more kept boxes than max_gt, or on a malformed input.  With max_gt given and check=False
        nothing is read back; such scenes are then only flagged: input_info[b] = [n_masked, n_far, n_kept_boxes,
        status], status bit 1 = empty scene (its rows are [b, 0, ...]), kept > max_gt = boxes dropped beyond the
        capacity, -1 kept / status bits 2, 4, 8 = bad offsets, more than n_cap points, a draw out of range.
        Returns {'batch_size', 'points' (B * NUM_POINTS, 1 + C), 'gt_boxes' (when boxes were given), 'input_info'}; the
        voxel chain adds 'voxel_info' (B, 4) int32 = [n_masked, n_in_grid, n_voxels_before_cap, status] with the same status
        bits (1 = no voxel) and 16 = MAX_NUMBER_OF_VOXELS was reached, which is not an error (the reference caps silently);
        input_info then counts voxel rows."""
        dev = torch.device(device) if device is not None else None
        pts, offs, n_cap, bxs, boffs, bmax = self._inputs(points, gt_boxes, dev)
        dev = pts.device
        B, C, k = offs.numel() - 1, pts.shape[1], self.num_points
        if C < 3:
            raise ValueError("points need at least x, y, z")
        if draws is None and seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())   # CPU generator: no device read
        voxel_info = None
        if self.voxel is not None:
            pts, offs, n_cap, voxel_info = self._voxel_stage(pts, offs, n_cap, seed, draws)
        ws = workspace("pda_input_stage_workspace_bytes", (B, n_cap), "batch %d / n_cap %d out of range" % (B, n_cap), dev)
        out = torch.empty((B * k, 1 + C), dtype=torch.float32, device=dev)
        info = (torch.empty if bxs is not None else torch.zeros)((B, 4), dtype=torch.int32, device=dev)
        pick = perm1 = perm2 = None
        if draws is not None:
            pick = self._draw_rows(draws.get('pick'), B, k, dev, 'pick')
            perm1 = self._draw_rows(draws.get('perm1'), B, k, dev, 'perm1')
            if self.shuffle:
                perm2 = self._draw_rows(draws.get('perm2'), B, k, dev, 'perm2')
            seed = 0
        _call("pda_input_stage", pts, _chk(pts, "points", F32), _chk(offs, "offsets", torch.int64), pts.shape[0], B, C, n_cap,
              self._range_c, k, pick.data_ptr() if pick is not None else None, perm1.data_ptr() if perm1 is not None else None,
              perm2.data_ptr() if perm2 is not None else None, ctypes.c_uint64(seed & (2 ** 64 - 1)), int(self.shuffle),
              out.data_ptr(), info.data_ptr(), ws.data_ptr())
        ret = {'batch_size': B, 'points': out, 'input_info': info}
        if voxel_info is not None:
            ret['voxel_info'] = voxel_info
        host_info = None
        if bxs is not None:
            cap = max_gt if max_gt is not None else bmax
            gt = torch.empty((B, cap, bxs.shape[1]), dtype=torch.float32, device=dev)
            _call("pda_input_boxes", bxs, _chk(bxs, "gt_boxes", F32), _chk(boffs, "box_offsets", torch.int64), bxs.shape[0], B,
                  bxs.shape[1], cap, self._range_c_boxes(), self.min_num_corners if self.remove_outside_boxes else 0,
                  gt.data_ptr() if cap > 0 else None, info.data_ptr())
            if max_gt is None:
                host_info = info.cpu()
                kept = host_info[:, 2]
                cap = int(kept.max()) if B > 0 else 0
                gt = gt[:, :max(cap, 0)].contiguous()
            ret['gt_boxes'] = gt
        if check:
            if voxel_info is not None:
                raise_on_status(voxel_info.cpu(), _VOXEL_RULES)
            self._check(info.cpu() if host_info is None else host_info, max_gt if bxs is not None else None)
        return ret

    def _voxel_stage(self, pts, offs, n_cap, seed, draws):
        """pda_voxel_sample: -> the voxel rows (packed, offsets, their capacity a scene) and voxel_info."""
        sp = self.voxel
        dev = pts.device
        B, C = offs.numel() - 1, pts.shape[1]
        mean = self.sample_type == 'mean_vfe'
        v_cap = min(n_cap, sp.max_voxels)
        ws = sp.workspace(B, n_cap, sp.max_points if mean else 1, dev)
        rows = torch.empty((B * v_cap, C), dtype=torch.float32, device=dev)
        row_offs = torch.empty((B + 1,), dtype=torch.int64, device=dev)
        info = torch.empty((B, 4), dtype=torch.int32, device=dev)
        perm0 = poffs = None
        if draws is not None and self.shuffle_first:
            per_scene = draws.get('perm0')
            if per_scene is None or len(per_scene) != B:
                raise ValueError("draws needs 'perm0' with one array per scene")
            per_scene = [np.asarray(r.cpu() if isinstance(r, torch.Tensor) else r).reshape(-1).astype(np.int32) for r in per_scene]
            poffs = torch.from_numpy(offsets_of([r.size for r in per_scene])).to(dev)
            perm0 = torch.from_numpy(np.concatenate(per_scene + [np.zeros(1, np.int32)])).to(dev)     # never empty
        _call("pda_voxel_sample", pts, _chk(pts, "points", F32), _chk(offs, "offsets", torch.int64), pts.shape[0], B, C, n_cap,
              sp.range_c, sp.vsize_c, sp.grid_c, int(self.mask_points), sp.max_voxels, sp.max_points if mean else 1, int(mean),
              int(self.shuffle_first), perm0.data_ptr() if perm0 is not None else None,
              poffs.data_ptr() if poffs is not None else None, perm0.numel() - 1 if perm0 is not None else 0,
              ctypes.c_uint64((seed or 0) & (2 ** 64 - 1)), rows.data_ptr(), rows.shape[0], row_offs.data_ptr(), info.data_ptr(),
              ws.data_ptr())
        return rows, row_offs, v_cap, info

    def _range_c_boxes(self):
        return (ctypes.c_float * 6)(*self.point_cloud_range.tolist())

    @staticmethod
    def _check(info, max_gt):
        # the first scene whose kept-box count is an error of its own; a status bit of that scene or an earlier one goes first
        kept = info[:, 2].tolist()
        bad = next((b for b, n in enumerate(kept) if n < 0 or (max_gt is not None and n > max_gt)), len(kept))
        raise_on_status(info[:bad + 1], _INPUT_RULES)
        if bad < len(kept):
            if kept[bad] < 0:
                raise ValueError("scene %d: box offsets outside the packed boxes" % bad)
            raise ValueError("scene %d keeps %d boxes, more than max_gt=%d" % (bad, kept[bad], max_gt))

    @staticmethod
    def _draw_rows(rows, B, k, dev, name):
        if rows is None:
            raise ValueError("draws needs %r" % name)
        if isinstance(rows, torch.Tensor) and rows.is_cuda:
            t = rows.to(torch.int32).contiguous()
            if t.shape != (B, k):
                raise ValueError("draws[%r] must be (B, NUM_POINTS)" % name)
            return t
        a = np.zeros((B, k), np.int32)
        if len(rows) != B:
            raise ValueError("draws[%r] needs one row per scene" % name)
        for b, r in enumerate(rows):
            r = np.asarray(r.cpu() if isinstance(r, torch.Tensor) else r).reshape(-1)
            if r.size > k:
                raise ValueError("draws[%r][%d] holds more than NUM_POINTS entries" % (name, b))
            a[b, :r.size] = r
        return torch.from_numpy(a).to(dev)

    def _inputs(self, points, gt_boxes, dev):
        """-> packed points, offsets, n_cap, packed boxes, box offsets, largest raw box count (all on one device)."""
        if isinstance(points, tuple):
            pts, offs, n_cap = packed_form(points)
            bxs = boffs = None
            bmax = 0
            if gt_boxes is not None:
                if not isinstance(gt_boxes, tuple):
                    raise ValueError("device points take gt_boxes as (packed, box_offsets)")
                bxs, boffs = gt_boxes
                bmax = bxs.shape[0]
            return pts, offs, n_cap, bxs, boffs, bmax
        B = len(points)
        if B == 0:
            raise ValueError("empty batch")
        if gt_boxes is not None and len(gt_boxes) != B:
            raise ValueError("gt_boxes needs one array per scene")
        on_dev = [isinstance(p, torch.Tensor) and p.is_cuda for p in points]
        if all(on_dev):
            dev = points[0].device
        elif dev is None:
            dev = current_device()
        # one transfer: offsets | points (when every scene is on the host) | box offsets | boxes
        host_pts = not any(on_dev)
        if host_pts:
            packed, offs, n_cap, _ = pack_scenes(points)
            host = [offs, packed]
        else:
            pts = [torch.as_tensor(p).to(dev, torch.float32) for p in points]
            if any(p.dim() != 2 or p.shape[1] != pts[0].shape[-1] for p in pts):
                raise ValueError("every scene must be (n_i, C) with the same C")
            sizes = [p.shape[0] for p in pts]
            n_cap = max(max(sizes), 1)
            pts = torch.cat(pts, dim=0).contiguous()
            host = [offsets_of(sizes)]
        bmax = 0
        if gt_boxes is not None:
            boxes = [np.asarray(g.cpu().numpy() if isinstance(g, torch.Tensor) else g, np.float32) for g in gt_boxes]
            D = max((g.shape[1] for g in boxes if g.ndim == 2 and g.size), default=7)
            boxes = [g.reshape(-1, D) for g in boxes]
            bmax = max(g.shape[0] for g in boxes)
            host += [offsets_of([g.shape[0] for g in boxes]), np.concatenate(boxes, axis=0)]
        views = upload(host, dev)
        d_offs = views[0]
        if host_pts:
            pts = views[1]
        d_boffs, bxs = views[-2:] if gt_boxes is not None else (None, None)
        return pts, d_offs, n_cap, bxs, d_boffs, bmax


def from_config(cfg, training):
    """DataProcessor of a loaded yaml (pdanet_amd.config.load_yaml): DATA_CONFIG.DATA_PROCESSOR / POINT_CLOUD_RANGE /
    NUM_POINT_FEATURES."""
    dc = cfg['DATA_CONFIG']
    return DataProcessor(dc['DATA_PROCESSOR'], dc['POINT_CLOUD_RANGE'], training, dc['NUM_POINT_FEATURES'])


def collate_batch(batch_list, max_gt=None, device=None):
    """DatasetTemplate.collate_batch for scenes that are already processed (pcdet/datasets/dataset.py), on the GPU:
    'points' (n_i, C) get the batch column in front and are concatenated, 'gt_boxes' (m_i, D) are zero-padded to max_gt
    (None: the largest count, as the reference does) by the same kernel DataProcessor uses (pda_input_boxes, every box
    kept).  Host inputs (numpy, CPU tensors) are moved to `device` (default: the device of the first scene's points when
    they are a GPU tensor, else the current GPU).  Every other key is stacked as the reference does (np.stack; torch.stack
    when every value is a tensor), so non-numeric keys such as frame_id pass through."""
    B = len(batch_list)
    if B == 0:
        raise ValueError("empty batch")
    keys = list(batch_list[0].keys())
    if device is None:
        first = batch_list[0].get('points')
        device = first.device if isinstance(first, torch.Tensor) and first.is_cuda else current_device()
    dev = torch.device(device)
    ret = {}
    for key in keys:
        val = [d[key] for d in batch_list]
        if key == 'points':
            pts = [torch.as_tensor(v).to(dev, torch.float32) for v in val]
            ret[key] = torch.cat([torch.cat([torch.full((v.shape[0], 1), float(i), dtype=torch.float32, device=dev), v], dim=1)
                                  for i, v in enumerate(pts)], dim=0)
        elif key == 'gt_boxes':
            boxes = [torch.as_tensor(v).to(dev, torch.float32) for v in val]
            D = boxes[0].shape[-1]
            boxes = [b.reshape(-1, D) for b in boxes]
            counts = [b.shape[0] for b in boxes]
            cap = max(counts) if max_gt is None else int(max_gt)
            if max(counts) > cap:
                raise ValueError("a scene holds more than max_gt=%d boxes" % cap)
            packed = torch.cat(boxes, dim=0).contiguous()
            offs = torch.from_numpy(offsets_of(counts)).to(dev)
            gt = torch.empty((B, cap, D), dtype=torch.float32, device=dev)
            info = torch.empty((B, 4), dtype=torch.int32, device=dev)
            rng = (ctypes.c_float * 6)(*([0.0] * 6))        # min_num_corners 0: every box is kept, the range is not read
            _call("pda_input_boxes", packed, _chk(packed, "gt_boxes", F32), _chk(offs, "box_offsets", torch.int64), packed.shape[0],
                  B, D, cap, rng, 0, gt.data_ptr() if cap > 0 else None, info.data_ptr())
            ret[key] = gt
        elif all(isinstance(v, torch.Tensor) for v in val):
            ret[key] = torch.stack(val, dim=0)
        else:
            ret[key] = np.stack(val, axis=0)
    ret['batch_size'] = B
    return ret
