"""The training-time augmentor on the device: ragged raw scenes -> ragged augmented scenes, ready for DataProcessor.

The reference augments every scene on the host (pcdet/datasets/augmentor/data_augmentor.py DataAugmentor.forward and
database_sampler.py DataBaseSampler, called from pcdet/datasets/dataset.py prepare_data).  DataAugmentor reads the same
DATA_AUGMENTOR block and runs gt_sampling -> random_world_flip -> random_world_rotation -> random_world_scaling ->
limit_period and prepare_data's class filter for all scenes of a batch in four launches (csrc/augment.hip,
include/pda_train.h pda_augment).

What stays on the host is what decides, per batch, which objects are tried and how each scene is transformed -- the
plan: the sampler's pointer / permutation bookkeeping (kept across calls, as the reference keeps it), the flip / rotation
/ scaling draws and, with USE_ROAD_PLANE, the road-plane shift of every candidate.  It is built from host class ids
only and uploaded with one copy.  Everything that touches points or boxes -- the BEV collision test, the removal of
scene points inside the pasted boxes, the paste and the world transforms -- runs on the device.

Randomness: `plan=` takes the draws the reference made (exact reproduction); otherwise they come from a numpy Generator
seeded from torch's CPU generator, so torch.manual_seed makes a run reproducible.  The Generator's stream is not the
reference's legacy np.random stream.

A DATA_AUGMENTOR list that holds one of the six further steps -- random_world_translation, random_world_frustum_dropout,
random_local_translation, random_local_rotation, random_local_scaling, random_local_frustum_dropout -- takes another
path: the paste alone (pda_augment_paste), then every step in the order the yaml lists it as one ordered program on the
device (csrc/augment_steps.hip, pda_augment_steps).  A list of only the four steps above takes the path above, unchanged.

random_local_pyramid_aug (the SE-SSD part-aware step: pyramid dropout, sparsify and swap) is a step of that path too, as
the last step of the list: the program ends in a hold op that keeps class 0 and the headings as they are, and
pda_pyramid_aug runs on what it leaves, then limit_period and the class filter.

A scene the augmentor leaves without a box is only flagged (info[:, 3] bit 1): the reference's prepare_data draws
another scene there, which a batch-level loader has to decide for itself.
"""
import ctypes
import os
import pickle

import numpy as np
import torch

from .pointnet2_batch_cuda import F32, _call, _chk
from .stage_common import (STATUS_BAD_OFFSETS, STATUS_OVER_CAP, cfg_get, current_device, offsets_of, pack_scenes, packed_form,
                           raise_on_status, upload, workspace)

# info[:, 3] status bits (include/pda_train.h pda_augment) next to the two shared ones, and what check=True raises
STATUS_NO_BOX, STATUS_BAD_CAND, STATUS_BAD_PYRAMID_DRAW = 1, 8, 16
_RULES = [(STATUS_BAD_OFFSETS, ": offsets outside the packed points or boxes"),
          (STATUS_OVER_CAP, ": more than n_cap points, an output capacity exceeded, or (program path) more boxes than the cap or "
                            "than draws"),
          (STATUS_BAD_CAND, ": a candidate id outside the database or candidate groups out of order"),
          (STATUS_BAD_PYRAMID_DRAW, ": random_local_pyramid_aug with fewer draws than boxes or an invalid explicit draw (a keep "
                                    "list, a swap face or a swap partner)")]
MAX_CANDIDATES = 256
MAX_SCENE_BOXES = 256            # boxes per scene (its own plus the candidates) on the program path
_STEPS = ("gt_sampling", "random_world_flip", "random_world_rotation", "random_world_scaling")
# the steps of the program path and the parameters each cannot run without
_PROGRAM_STEPS = {"random_world_translation": ("NOISE_TRANSLATE_STD", "ALONG_AXIS_LIST"),
                  "random_world_frustum_dropout": ("INTENSITY_RANGE", "DIRECTION"),
                  "random_local_translation": ("LOCAL_TRANSLATION_RANGE", "ALONG_AXIS_LIST"),
                  "random_local_rotation": ("LOCAL_ROT_ANGLE",),
                  "random_local_scaling": ("LOCAL_SCALE_RANGE",),
                  "random_local_frustum_dropout": ("INTENSITY_RANGE", "DIRECTION"),
                  "random_local_pyramid_aug": ("DROP_PROB", "SPARSIFY_PROB", "SPARSIFY_MAX_NUM", "SWAP_PROB", "SWAP_MAX_NUM")}
# op codes of pda_augment_steps (include/pda_train.h); OP_HOLD ends the program in front of pda_pyramid_aug
OP_FLIP_X, OP_FLIP_Y, OP_ROT, OP_SCALE, OP_TRANS, OP_WDROP, OP_LTRANS, OP_LROT, OP_LSCALE, OP_LDROP, OP_HOLD = range(11)
MAX_SPARSIFY_NUM = 1024          # SPARSIFY_MAX_NUM at most (pda_pyramid_aug)
# the per-box rows of random_local_pyramid_aug's plan, in the row order of pda_pyramid_aug's draws_f64 / draws_i32
_PYRAMID_F64 = ("pyramid_drop_u", "pyramid_sparsify_u", "pyramid_swap_u", "pyramid_swap_face_u", "pyramid_swap_partner_u")
_PYRAMID_I32 = ("pyramid_drop_face", "pyramid_sparsify_face", "pyramid_swap_face", "pyramid_swap_partner")
_AXES = {"x": 0, "y": 1, "z": 2}
_DIRECTIONS = {"top": 0, "bottom": 1, "left": 2, "right": 3}


def class_ids(gt_names, class_names):
    """prepare_data's class column: CLASS_NAMES.index(name) + 1, and 0 for a name outside CLASS_NAMES."""
    names = list(class_names)
    return np.array([names.index(n) + 1 if n in names else 0 for n in gt_names], np.int32)


class GtDatabase:
    """The gt_sampling database on the device: every object of CLASS_NAMES in class order, its points relative to its
    box centre (as the reference stores them), its box (float32), its centre box3d_lidar[:3] (float64) and class id.
    Host copies of the boxes and sizes stay for the plan."""

    def __init__(self, class_names, boxes, points, device=None):
        self.class_names = list(class_names)
        dev = torch.device(device) if device is not None else current_device()
        self.start, self.count = {}, {}
        box_rows, pts, cls = [], [], []
        for ci, name in enumerate(self.class_names):
            b = np.asarray(boxes.get(name, np.zeros((0, 7))), np.float64)
            b = b.reshape(-1, b.shape[-1]) if b.size else np.zeros((0, 7))
            p = list(points.get(name, []))
            if b.shape[1] != 7:
                raise NotImplementedError("database boxes with %d values: boxes with velocities are not supported" % b.shape[1])
            if len(p) != b.shape[0]:
                raise ValueError("class %s: %d boxes but %d point sets" % (name, b.shape[0], len(p)))
            self.start[name] = sum(len(x) for x in box_rows)
            self.count[name] = b.shape[0]
            box_rows.append(b)
            pts.extend(np.asarray(x, np.float32) for x in p)
            cls.extend([ci + 1] * b.shape[0])
        centre = np.concatenate(box_rows, 0) if box_rows else np.zeros((0, 7))
        self.n_obj = centre.shape[0]
        C = pts[0].shape[1] if pts else 4
        if any(x.ndim != 2 or x.shape[1] != C for x in pts):
            raise ValueError("every object needs (n, C) points with the same C")
        self.num_point_features = C
        self.sizes = np.array([x.shape[0] for x in pts], np.int64)
        self.host_boxes = centre.astype(np.float32)                # sampled_boxes = box3d_lidar.astype(np.float32)
        offs = offsets_of(self.sizes)
        allp = np.concatenate(pts, 0) if pts else np.zeros((0, C), np.float32)
        self.device = dev
        self.points = torch.from_numpy(np.ascontiguousarray(allp)).to(dev)
        self.offsets = torch.from_numpy(offs).to(dev)
        self.boxes = torch.from_numpy(np.ascontiguousarray(self.host_boxes)).to(dev)
        self.centre = torch.from_numpy(np.ascontiguousarray(centre[:, :3])).to(dev)
        self.classes = torch.from_numpy(np.array(cls, np.int32)).to(dev)

    @classmethod
    def from_arrays(cls, class_names, boxes, points, device=None):
        """boxes: {class name: (n, 7) box3d_lidar (float64 as the dbinfos hold them)}; points: {class name: [n arrays
        (n_i, C) of object points relative to the box centre]}."""
        return cls(class_names, boxes, points, device)

    @classmethod
    def from_device(cls, class_names, boxes, points, offsets, ids):
        """A database whose object points are on the device already (frame_stage.GtDatabaseBuilder.finish): boxes as for
        from_arrays; points (rows, C) float32 device tensor holding object o at rows [offsets[o], offsets[o + 1]), offsets
        a host int64 array; ids: the objects taken, class by class in CLASS_NAMES order (one per box).  The points are
        gathered on the device."""
        self = cls.__new__(cls)
        self.class_names = list(class_names)
        self.start, self.count = {}, {}
        box_rows, cls_ids = [], []
        for ci, name in enumerate(self.class_names):
            b = np.asarray(boxes.get(name, np.zeros((0, 7))), np.float64)
            b = b.reshape(-1, b.shape[-1]) if b.size else np.zeros((0, 7))
            if b.shape[1] != 7:
                raise NotImplementedError("database boxes with %d values: boxes with velocities are not supported" % b.shape[1])
            self.start[name] = sum(len(x) for x in box_rows)
            self.count[name] = b.shape[0]
            box_rows.append(b)
            cls_ids.extend([ci + 1] * b.shape[0])
        centre = np.concatenate(box_rows, 0) if box_rows else np.zeros((0, 7))
        ids = np.asarray(ids, np.int64).reshape(-1)
        offsets = np.asarray(offsets, np.int64).reshape(-1)
        if ids.size != centre.shape[0]:
            raise ValueError("%d boxes but %d object ids" % (centre.shape[0], ids.size))
        if ids.size and (ids.min() < 0 or ids.max() >= offsets.size - 1):
            raise ValueError("an object id outside the packed points")
        if not points.is_cuda or points.dim() != 2 or points.dtype != torch.float32:
            raise ValueError("points must be a (rows, C) float32 device tensor")
        self.n_obj = centre.shape[0]
        self.num_point_features = points.shape[1]
        self.sizes = (offsets[ids + 1] - offsets[ids]).astype(np.int64)
        self.host_boxes = centre.astype(np.float32)
        offs = offsets_of(self.sizes)
        # the source row of every database row: object starts repeated, plus the position inside the object
        rows = np.repeat(offsets[ids] - offs[:-1], self.sizes) + np.arange(offs[-1], dtype=np.int64)
        dev = self.device = points.device
        self.points = points.index_select(0, torch.from_numpy(rows).to(dev)).contiguous()
        self.offsets = torch.from_numpy(offs).to(dev)
        self.boxes = torch.from_numpy(np.ascontiguousarray(self.host_boxes)).to(dev)
        self.centre = torch.from_numpy(np.ascontiguousarray(centre[:, :3])).to(dev)
        self.classes = torch.from_numpy(np.array(cls_ids, np.int32)).to(dev)
        return self

    @classmethod
    def from_dbinfos(cls, root_path, sampler_cfg, class_names, device=None):
        """The database DataBaseSampler.__init__ builds: the DB_INFO_PATH pickles under root_path, PREPARE applied
        (filter_by_min_points, filter_by_difficulty), points from the per-object .bin files or, with
        USE_SHARED_MEMORY, from DB_DATA_PATH[0] sliced by global_data_offset."""
        db_infos = {name: [] for name in class_names}
        for rel in sampler_cfg['DB_INFO_PATH']:
            with open(os.path.join(str(root_path), rel), 'rb') as f:
                infos = pickle.load(f)
            for name in class_names:
                db_infos[name].extend(infos[name])
        for func, val in cfg_get(sampler_cfg, 'PREPARE', {}).items():
            if func == 'filter_by_min_points':
                db_infos = _filter_by_min_points(db_infos, val)
            elif func == 'filter_by_difficulty':
                db_infos = {k: [i for i in v if i['difficulty'] not in val] for k, v in db_infos.items()}
            else:
                raise NotImplementedError("PREPARE step %r" % func)
        C = int(sampler_cfg['NUM_POINT_FEATURES'])
        data = None
        if cfg_get(sampler_cfg, 'USE_SHARED_MEMORY', False):
            data = np.load(os.path.join(str(root_path), sampler_cfg['DB_DATA_PATH'][0]))
        boxes, points = {}, {}
        for name in class_names:
            infos = db_infos[name]
            boxes[name] = (np.stack([np.asarray(i['box3d_lidar'], np.float64) for i in infos]) if infos
                           else np.zeros((0, 7)))
            pl = []
            for i in infos:
                if data is not None:
                    s, e = i['global_data_offset']
                    pl.append(np.array(data[s:e], np.float32).reshape(-1, C))
                else:
                    pl.append(np.fromfile(os.path.join(str(root_path), i['path']), dtype=np.float32).reshape(-1, C))
            points[name] = pl
        return cls(class_names, boxes, points, device)


def _filter_by_min_points(db_infos, min_gt_points_list):
    for name_num in min_gt_points_list:
        name, min_num = name_num.split(':')
        min_num = int(min_num)
        if min_num > 0 and name in db_infos:
            db_infos[name] = [i for i in db_infos[name] if i['num_points_in_gt'] >= min_num]
    return db_infos


# plan key, op code, one draw per box (else one per scene)
_PLAN_KEYS = (("translation", OP_TRANS, False), ("world_dropout", OP_WDROP, False), ("local_translation", OP_LTRANS, True),
              ("local_rotation", OP_LROT, True), ("local_scaling", OP_LSCALE, True), ("local_dropout", OP_LDROP, True))


class _Group:
    def __init__(self, name, num, class_id, length):
        self.name, self.num, self.class_id = name, num, class_id
        self.pointer, self.indices = length, np.arange(length)


class DataAugmentor:
    """DATA_AUGMENTOR of a reference-shaped yaml (AUG_CONFIG_LIST minus DISABLE_AUG_LIST): gt_sampling,
    random_world_flip, random_world_rotation, random_world_scaling, random_world_translation,
    random_world_frustum_dropout, random_local_translation, random_local_rotation, random_local_scaling and
    random_local_frustum_dropout, in the order the list gives, each at most once; gt_sampling must come first (the
    transforms follow the paste).  random_local_pyramid_aug runs as the LAST step of the list (its place in
    pointpillar_pyramid_aug.yaml); anywhere else it raises NotImplementedError.  Its SPARSIFY_MAX_NUM is at most 1024
    (an explicit keep list is validated rank against rank on the device) and its point rows need C >= 4; a larger
    SPARSIFY_MAX_NUM raises ValueError.  Any other step (random_image_flip) raises NotImplementedError.

    An entry of one of the last seven steps that lacks a parameter the step needs cannot be run and raises
    NotImplementedError naming the step and the key: NOISE_TRANSLATE_STD and ALONG_AXIS_LIST (world translation),
    LOCAL_TRANSLATION_RANGE and ALONG_AXIS_LIST (local translation), LOCAL_ROT_ANGLE, LOCAL_SCALE_RANGE, INTENSITY_RANGE
    and DIRECTION (both dropouts), DROP_PROB, SPARSIFY_PROB, SPARSIFY_MAX_NUM, SWAP_PROB and SWAP_MAX_NUM (pyramid aug).

    A list of only the first four steps runs as pda_augment (flip, rotation, scaling in that fixed place); a list with
    one of the others runs the paste, then `program`: one op per step, axis or direction, in yaml order.

    random_world_frustum_dropout: the reference drops the box rows but not their gt_names, so its own class mask no
    longer fits once a box is dropped; here a dropped box goes together with its class."""

    def __init__(self, aug_cfg, class_names, database=None):
        self.class_names = list(class_names)
        cfg_list = aug_cfg if isinstance(aug_cfg, list) else aug_cfg['AUG_CONFIG_LIST']
        disabled = [] if isinstance(aug_cfg, list) else list(cfg_get(aug_cfg, 'DISABLE_AUG_LIST', []))
        self.sampler_cfg = None
        self.flip_axes, self.flip_prob = [], 0.5
        self.rot_range, self.rot_prob = None, 1.0
        self.scale_range, self.scale_prob = None, 1.0
        self.pyramid = None              # random_local_pyramid_aug's parameters
        seen = []
        steps = []                       # (op code, arg, step name, its parameters), in yaml order
        for cfg in cfg_list:
            name = cfg['NAME']
            if name in disabled:
                continue
            if name not in _STEPS and name not in _PROGRAM_STEPS:
                raise NotImplementedError("DATA_AUGMENTOR step %r has no device implementation" % name)
            for key in _PROGRAM_STEPS.get(name, ()):
                if key not in cfg:
                    raise NotImplementedError("DATA_AUGMENTOR step %r cannot run without %s" % (name, key))
            if name in seen:
                raise NotImplementedError("DATA_AUGMENTOR step %r appears twice" % name)
            if name == 'gt_sampling' and seen:
                raise NotImplementedError("gt_sampling must be the first DATA_AUGMENTOR step")
            if self.pyramid is not None:
                raise NotImplementedError("random_local_pyramid_aug runs as the last DATA_AUGMENTOR step only: %r follows it" % name)
            seen.append(name)
            if name == 'gt_sampling':
                self.sampler_cfg = cfg
            elif name == 'random_world_flip':
                self.flip_axes = list(cfg['ALONG_AXIS_LIST'])
                if any(a not in ('x', 'y') for a in self.flip_axes):
                    raise ValueError("random_world_flip takes the axes 'x' and 'y'")
                self.flip_prob = float(cfg_get(cfg, 'ENABLE_PROB', 0.5))
                steps += [(OP_FLIP_X if a == 'x' else OP_FLIP_Y, 0, name, None) for a in self.flip_axes]
            elif name == 'random_world_rotation':
                r = cfg['WORLD_ROT_ANGLE']
                self.rot_range = [float(r[0]), float(r[1])] if isinstance(r, (list, tuple)) else [-float(r), float(r)]
                self.rot_prob = float(cfg_get(cfg, 'ENABLE_PROB', 1.0))
                steps.append((OP_ROT, 0, name, None))
            elif name == 'random_world_scaling':
                self.scale_range = [float(x) for x in cfg['WORLD_SCALE_RANGE']]
                self.scale_prob = float(cfg_get(cfg, 'ENABLE_PROB', 1.0))
                steps.append((OP_SCALE, 0, name, None))
            elif name in ('random_world_translation', 'random_local_translation'):
                axes = list(cfg['ALONG_AXIS_LIST'])
                if any(a not in _AXES for a in axes):
                    raise ValueError("%s takes the axes 'x', 'y' and 'z'" % name)
                if name == 'random_world_translation':
                    std = float(cfg['NOISE_TRANSLATE_STD'])
                    if std != 0:                 # the reference returns before any draw
                        steps += [(OP_TRANS, _AXES[a], name, std) for a in axes]
                else:
                    r = [float(x) for x in cfg['LOCAL_TRANSLATION_RANGE']]
                    steps += [(OP_LTRANS, _AXES[a], name, r) for a in axes]
            elif name == 'random_local_rotation':
                r = cfg['LOCAL_ROT_ANGLE']
                r = [float(r[0]), float(r[1])] if isinstance(r, (list, tuple)) else [-float(r), float(r)]
                steps.append((OP_LROT, 0, name, r))
            elif name == 'random_local_scaling':
                r = [float(x) for x in cfg['LOCAL_SCALE_RANGE']]
                if r[1] - r[0] >= 1e-3:          # the reference skips the step as a whole, without a draw
                    steps.append((OP_LSCALE, 0, name, r))
            elif name == 'random_local_pyramid_aug':
                self.pyramid = dict(drop_prob=float(cfg['DROP_PROB']), sparsify_prob=float(cfg['SPARSIFY_PROB']),
                                    sparsify_max=int(cfg['SPARSIFY_MAX_NUM']), swap_prob=float(cfg['SWAP_PROB']),
                                    swap_max=int(cfg['SWAP_MAX_NUM']))
                if not 0 <= self.pyramid['sparsify_max'] <= MAX_SPARSIFY_NUM or self.pyramid['swap_max'] < 0:
                    raise ValueError("random_local_pyramid_aug takes SPARSIFY_MAX_NUM in [0, %d] and SWAP_MAX_NUM >= 0" % MAX_SPARSIFY_NUM)
            else:
                dirs = list(cfg['DIRECTION'])
                if any(d not in _DIRECTIONS for d in dirs):
                    raise ValueError("%s takes the directions 'top', 'bottom', 'left' and 'right'" % name)
                r = [float(x) for x in cfg['INTENSITY_RANGE']]
                code = OP_WDROP if name == 'random_world_frustum_dropout' else OP_LDROP
                steps += [(code, _DIRECTIONS[d], name, r) for d in dirs]
        # the ordered program, or None: a list of the four first steps alone keeps the pda_augment path
        self.program = steps if any(n in _PROGRAM_STEPS for n in seen) else None
        if self.program is not None and sum(1 for st in steps if st[0] == OP_WDROP) > 4:
            raise ValueError("random_world_frustum_dropout takes at most four directions")
        if self.program is not None and len(steps) + (self.pyramid is not None) > 32:      # the hold op is one of the 32
            raise ValueError("more than 32 ops in the DATA_AUGMENTOR program")
        self.database = database
        self.groups, self.limit_whole_scene, self.use_road_plane = [], False, False
        self.remove_extra_width = np.zeros(3, np.float32)
        if self.sampler_cfg is not None:
            if database is None:
                raise ValueError("gt_sampling needs a GtDatabase")
            if database.class_names != self.class_names:
                raise ValueError("the database was built for other CLASS_NAMES")
            if cfg_get(self.sampler_cfg, 'DATABASE_WITH_FAKELIDAR', False):
                raise NotImplementedError("DATABASE_WITH_FAKELIDAR")
            self.limit_whole_scene = bool(cfg_get(self.sampler_cfg, 'LIMIT_WHOLE_SCENE', False))
            self.use_road_plane = bool(cfg_get(self.sampler_cfg, 'USE_ROAD_PLANE', False))
            self.remove_extra_width = np.asarray(self.sampler_cfg['REMOVE_EXTRA_WIDTH'], np.float32).reshape(3)
            names = {}
            for x in self.sampler_cfg['SAMPLE_GROUPS']:
                name, num = x.split(':')
                if name not in self.class_names:
                    continue
                names[name] = int(num)          # the reference keeps one group per class (a dict), the last count wins
            for name, num in names.items():
                self.groups.append(_Group(name, num, self.class_names.index(name) + 1, database.count[name]))
        self._rew_c = (ctypes.c_float * 3)(*self.remove_extra_width.tolist())

    # ---- the plan ----------------------------------------------------------------------------------------------------
    def sample_candidates(self, gt_classes, permutation):
        """DataBaseSampler's bookkeeping for a batch: per scene, the database ids tried by each class group in
        SAMPLE_GROUPS order, and their groups.  permutation(n) draws the new order when a class's pointer wraps.
        Advances the sampler state, as the reference does."""
        cand, group = [], []
        for cls in gt_classes:
            cls = np.asarray(cls).reshape(-1)
            ids, grp = [], []
            for g, st in enumerate(self.groups):
                num = st.num - int((cls == st.class_id).sum()) if self.limit_whole_scene else st.num
                if num <= 0:
                    continue
                length = self.database.count[st.name]
                if st.pointer >= length:
                    st.indices = np.asarray(permutation(length))
                    st.pointer = 0
                sel = st.indices[st.pointer:st.pointer + num]
                st.pointer += num
                ids.extend((self.database.start[st.name] + sel).tolist())
                grp.extend([g] * len(sel))
            cand.append(np.array(ids, np.int32))
            group.append(np.array(grp, np.int32))
        return cand, group

    def make_plan(self, gt_classes, rng=None):
        """The draws of one batch from a numpy Generator (default: seeded from torch's CPU generator): gt_sampling's
        permutations, then per scene flip x / flip y, rotation, scaling, each behind its ENABLE_PROB.  On the program
        path also: translation (B, axes) normal(0, NOISE_TRANSLATE_STD), world_dropout (B, directions), and for the local
        steps one row of D draws per scene and sub-step -- local_translation (B, axes, D), local_rotation (B, D),
        local_scaling (B, D), local_dropout (B, directions, D) -- with D = the most boxes a scene can hold (its own plus
        its candidates): how many survive the collision test is known on the device only, and the draws are i.i.d.
        With random_local_pyramid_aug also, each (B, D): pyramid_drop_face and pyramid_sparsify_face (integers 0..5),
        pyramid_drop_u, pyramid_sparsify_u, pyramid_swap_u, pyramid_swap_face_u and pyramid_swap_partner_u (uniform [0, 1))
        and pyramid_sparsify_key (uint64); the explicit pyramid_sparsify_keep / pyramid_swap_face / pyramid_swap_partner
        are never drawn."""
        if rng is None:
            rng = np.random.default_rng(int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()))
        B = len(gt_classes)
        plan = {}
        if self.groups:
            plan['cand'], plan['cand_group'] = self.sample_candidates(gt_classes, rng.permutation)
        fx, fy, ang, scl = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B), np.ones(B, np.float32)
        for b in range(B):
            for ax in self.flip_axes:
                on = rng.random() < self.flip_prob
                if ax == 'x':
                    fx[b] = on
                else:
                    fy[b] = on
            if self.rot_range is not None and rng.random() < self.rot_prob:
                ang[b] = rng.uniform(self.rot_range[0], self.rot_range[1])
            if self.scale_range is not None and self.scale_range[1] - self.scale_range[0] >= 1e-3 and rng.random() < self.scale_prob:
                scl[b] = np.float32(rng.uniform(self.scale_range[0], self.scale_range[1]))
        plan.update(flip_x=fx, flip_y=fy, angle=ang, scale=scl)
        if self.program is not None:
            cand = plan.get('cand') or [()] * B
            D = max([len(np.asarray(gt_classes[b]).reshape(-1)) + len(cand[b]) for b in range(B)] + [0])
            for key, code, per_box in _PLAN_KEYS:
                ops = [st for st in self.program if st[0] == code]
                if not ops:
                    continue
                shape = (B, len(ops), D) if per_box else (B, len(ops))
                if code == OP_TRANS:
                    val = rng.normal(0.0, ops[0][3], shape)
                else:
                    val = rng.uniform(ops[0][3][0], ops[0][3][1], shape)
                plan[key] = val[:, 0] if code in (OP_LROT, OP_LSCALE) else val
            if self.pyramid is not None:
                plan.update(pyramid_drop_face=rng.integers(0, 6, (B, D)), pyramid_drop_u=rng.random((B, D)),
                            pyramid_sparsify_face=rng.integers(0, 6, (B, D)), pyramid_sparsify_u=rng.random((B, D)),
                            pyramid_sparsify_key=rng.integers(0, 2 ** 64, (B, D), dtype=np.uint64),
                            pyramid_swap_u=rng.random((B, D)), pyramid_swap_face_u=rng.random((B, D)),
                            pyramid_swap_partner_u=rng.random((B, D)))
        return plan

    def _pyramid_draws(self, plan, B):
        """The pyramid rows of the plan as pda_pyramid_aug takes them: draws_f64 (B, 5, D), draws_i32 (B, 4, D), keys
        (B, D) uint64, keep (B, D, 1 + SPARSIFY_MAX_NUM) int32 [length, ranks] (empty without pyramid_sparsify_keep in the
        plan), n_draws (B, 3) int32 and D.  A row may be
        shorter than D; the rows of a scene that follow another in length are cut or padded to it (a missing override
        is -1, a missing face u or key 0)."""
        smax = self.pyramid['sparsify_max']
        rows = {}
        for key in _PYRAMID_F64 + _PYRAMID_I32 + ("pyramid_sparsify_key",):
            val = plan.get(key)
            if val is None:
                if key in ("pyramid_swap_face", "pyramid_swap_partner", "pyramid_swap_face_u", "pyramid_swap_partner_u",
                           "pyramid_sparsify_key"):
                    continue
                raise ValueError("the plan lacks %r" % key)
            if len(val) != B:
                raise ValueError("plan[%r] needs one entry per scene" % key)
            rows[key] = [np.asarray(r).reshape(-1) for r in val]
        n = np.zeros((B, 3), np.int32)
        for j, (a, c) in enumerate((("pyramid_drop_u", "pyramid_drop_face"), ("pyramid_sparsify_u", "pyramid_sparsify_face"),
                                    ("pyramid_swap_u", None))):
            for b in range(B):
                n[b, j] = len(rows[a][b])
                if c is not None and len(rows[c][b]) != n[b, j]:
                    raise ValueError("plan[%r][%d] and plan[%r][%d] differ in length" % (a, b, c, b))
        D = int(n.max()) if B else 0
        if D > MAX_SCENE_BOXES:
            raise ValueError("more than %d draws in one row of random_local_pyramid_aug" % MAX_SCENE_BOXES)
        W = max(D, 1)
        f64 = np.zeros((B, 5, W), np.float64)
        i32 = np.zeros((B, 4, W), np.int32)
        i32[:, 2:] = -1
        keys = np.zeros((B, W), np.uint64)
        keep_rows = plan.get("pyramid_sparsify_keep")
        # without explicit lists nothing is built or uploaded: the kernel takes a null pointer and uses the keys
        keep = np.zeros((B, W, 1 + smax) if keep_rows is not None else (0, 0, 0), np.int32)
        if keep_rows is not None and len(keep_rows) != B:
            raise ValueError("plan['pyramid_sparsify_keep'] needs one entry per scene")
        for b in range(B):
            for j, key in enumerate(_PYRAMID_F64):
                if key in rows:
                    r = rows[key][b][:n[b, min(j, 2)]]
                    f64[b, j, :len(r)] = r
            for j, key in enumerate(_PYRAMID_I32):
                if key in rows:
                    r = rows[key][b][:n[b, min(j, 2)]]
                    i32[b, j, :len(r)] = r
            if "pyramid_sparsify_key" in rows:
                r = rows["pyramid_sparsify_key"][b][:n[b, 1]]
                keys[b, :len(r)] = r.astype(np.uint64)
            if keep_rows is not None:
                if len(keep_rows[b]) > n[b, 1]:
                    raise ValueError("plan['pyramid_sparsify_keep'][%d] holds more lists than sparsify draws" % b)
                for j, lst in enumerate(keep_rows[b]):
                    lst = np.asarray(lst, np.int64).reshape(-1)
                    if len(lst) == 0:
                        continue
                    # a list of another length than SPARSIFY_MAX_NUM is invalid: the device flags it by its length
                    keep[b, j, 0] = len(lst)
                    keep[b, j, 1:1 + min(len(lst), smax)] = lst[:smax]
        return f64, i32, keys.view(np.int64), keep, n, D

    def _program_draws(self, plan, B, fx, fy, angle, scale):
        """The plan as pda_augment_steps takes it: ops (n_ops, 2) int32, scene_draws (B, n_ops) float64 and box_draws
        (B, local ops, D) float64, draw j of a row for the j-th box alive at that op."""
        n_ops = len(self.program)
        ops = np.array([[st[0], st[1]] for st in self.program], np.int32).reshape(n_ops, 2)
        scene = np.zeros((B, n_ops), np.float64)
        local = [i for i, st in enumerate(self.program) if st[0] >= OP_LTRANS]
        rows = {}
        for key, code, per_box in _PLAN_KEYS:
            at = [i for i, st in enumerate(self.program) if st[0] == code]
            if not at:
                continue
            if key not in plan:
                raise ValueError("the plan lacks %r" % key)
            val = plan[key]
            if len(val) != B:
                raise ValueError("plan[%r] needs one entry per scene" % key)
            for b in range(B):
                row = val[b]
                if per_box:
                    sub = [row] if len(at) == 1 and np.ndim(row) == 1 and not isinstance(row, (list, tuple)) else list(row)
                    if len(sub) != len(at):
                        raise ValueError("plan[%r][%d] needs %d rows of draws" % (key, b, len(at)))
                    for i, r in zip(at, sub):
                        rows[(b, i)] = np.asarray(r, np.float64).reshape(-1)
                else:
                    r = np.asarray(row, np.float64).reshape(-1)
                    if len(r) != len(at):
                        raise ValueError("plan[%r][%d] needs %d draws" % (key, b, len(at)))
                    scene[b, at] = r
        for i, st in enumerate(self.program):
            if st[0] == OP_FLIP_X:
                scene[:, i] = fx
            elif st[0] == OP_FLIP_Y:
                scene[:, i] = fy
            elif st[0] == OP_ROT:
                scene[:, i] = angle
            elif st[0] == OP_SCALE:
                scene[:, i] = scale.astype(np.float64)
        D = max([len(r) for r in rows.values()] + [0])
        if D > MAX_SCENE_BOXES:
            raise ValueError("more than %d draws in one row of a local step" % MAX_SCENE_BOXES)
        box = np.zeros((B, max(len(local), 1), max(D, 1)), np.float64)
        for (b, i), r in rows.items():
            box[b, local.index(i), :len(r)] = r
        return ops, scene, box, D

    def _mv_height(self, ids, road_plane, calib):
        """put_boxes_on_road_planes for the candidate boxes (each row on its own, so every candidate gets the shift
        it would get if accepted)."""
        boxes = self.database.host_boxes[ids].copy()
        a, b, c, d = road_plane
        center_cam = calib.lidar_to_rect(boxes[:, 0:3])
        cur_height_cam = (-d - a * center_cam[:, 0] - c * center_cam[:, 2]) / b
        center_cam[:, 1] = cur_height_cam
        cur_lidar_height = calib.rect_to_lidar(center_cam)[:, 2]
        return np.asarray(boxes[:, 2] - boxes[:, 5] / 2 - cur_lidar_height, np.float64)

    # ------------------------------------------------------------------------------------------------------------------
    def __call__(self, points, gt_boxes, gt_classes, plan=None, rng=None, road_planes=None, calib=None, check=True):
        """points: a list of B (n_i, C) arrays (host), or a tuple (packed (n_total, C) float32, offsets (B + 1) int64,
        n_cap) of device tensors.  gt_boxes: a list of B (m_i, 7) arrays, or a tuple (packed (m_total, 7) float32,
        box_offsets (B + 1) int64) of device tensors.  gt_classes: per scene, the host class ids of its boxes
        (class_ids(gt_names, CLASS_NAMES): 0 = a name outside CLASS_NAMES).
        plan: dict(cand=, cand_group=, flip_x=, flip_y=, angle=, scale=) -- cand / cand_group per scene (database ids
        in the order the sampler tried them, their group index); flip_x / flip_y 0/1, angle (0 = no rotation), scale
        (1 = no scaling) per scene.  On the program path also, per scene: translation (one offset per axis of
        random_world_translation's ALONG_AXIS_LIST, in list order), world_dropout (one intensity per DIRECTION), and for
        the local steps rows of per-box draws -- local_translation (axes, n), local_rotation (n), local_scaling (n),
        local_dropout (directions, n); rows may differ in length between scenes and sub-steps.  Draw j of a row belongs
        to the j-th box alive at that sub-step, in order (the scene's own boxes, then the accepted candidates, minus what
        a world dropout removed): the order in which the reference consumes np.random.uniform.  A scene with more alive
        boxes than draws in a row, or more than 256 boxes, is flagged (status 4) and written empty.
        With random_local_pyramid_aug also, per scene, rows of per-box draws: pyramid_drop_face (0..5) and pyramid_drop_u
        (draw j for box j of the boxes alive there, class 0 included); pyramid_sparsify_face, pyramid_sparsify_u and
        optionally pyramid_sparsify_key (uint64) and pyramid_sparsify_keep (a list per slot: SPARSIFY_MAX_NUM ranks into
        the pyramid's points in scene order, np.random.choice's result, or empty = the key decides), draw j for the j-th
        box not dropped; pyramid_swap_u and optionally pyramid_swap_face_u / pyramid_swap_partner_u in [0, 1) (index
        floor(u * k) among the k valid options in ascending order) or the explicit pyramid_swap_face (a face or -1) /
        pyramid_swap_partner (an index among the boxes in front of the swap, or -1), draw j for the j-th box neither
        dropped nor selected by the sparsify.  A scene with fewer draws than boxes in a row or an invalid explicit draw
        is flagged (status 16) and written empty.
        None: drawn by make_plan(gt_classes, rng), which advances the sampler.
        road_planes / calib: per scene, required by USE_ROAD_PLANE (the reference's road_plane [a, b, c, d] and a
        calibration with lidar_to_rect / rect_to_lidar).
        check: read info once and raise ValueError on malformed input (bad offsets, over capacity, a bad candidate).
        With check=False and device inputs nothing is read back.
        Returns ((points (rows, C), offsets (B + 1), n_cap), (boxes (rows, 8) [x, y, z, dx, dy, dz, heading, class],
        box_offsets (B + 1)), info (B, 4) int32 [points out, boxes out, accepted samples, status]); the first two feed
        DataProcessor.__call__ as they are."""
        B = len(gt_classes)
        if plan is None:
            plan = self.make_plan(gt_classes, rng)
        dev_in = isinstance(points, tuple)
        if dev_in:
            if not (isinstance(gt_boxes, tuple) and points[0].is_cuda and points[1].is_cuda):
                raise ValueError("device points take gt_boxes as a (packed, box_offsets) tuple of device tensors")
            pts, offs, n_cap = packed_form(points)
            bxs7, boffs = gt_boxes
            dev = pts.device
            if offs.numel() != B + 1 or boffs.numel() != B + 1:
                raise ValueError("offsets need B + 1 entries")
            if bxs7.dim() != 2 or bxs7.shape[1] != 7:
                raise NotImplementedError("boxes with more than 7 values (velocities) are not supported")
            n_total, C, m_total = pts.shape[0], pts.shape[1], bxs7.shape[0]
        else:
            if len(points) != B or len(gt_boxes) != B:
                raise ValueError("points, gt_boxes and gt_classes need one entry per scene")
            packed, offs_h, n_cap, C = pack_scenes(points)
            bl = [np.asarray(g, np.float32).reshape(len(g), -1) if len(g) else np.zeros((0, 7), np.float32) for g in gt_boxes]
            if any(g.shape[1] != 7 for g in bl):
                raise NotImplementedError("boxes with more than 7 values (velocities) are not supported")
            n_total, m_total = packed.shape[0], sum(len(g) for g in bl)
            dev = self.database.device if self.database is not None else current_device()
        cls_rows = [np.asarray(c, np.int32).reshape(-1) for c in gt_classes]
        if sum(len(c) for c in cls_rows) != m_total:
            raise ValueError("gt_classes needs one class id per box")
        db = self.database
        if db is not None and db.num_point_features != C:
            raise ValueError("the database holds %d point features, the scenes %d" % (db.num_point_features, C))

        # ---- the plan as arrays --------------------------------------------------------------------------------------
        cand_rows = plan.get('cand') if self.groups else None
        cand_rows = cand_rows if cand_rows is not None else [np.zeros(0, np.int32)] * B
        grp_rows = plan.get('cand_group') if self.groups else None
        grp_rows = grp_rows if grp_rows is not None else [np.zeros(0, np.int32)] * B
        if len(cand_rows) != B or len(grp_rows) != B:
            raise ValueError("plan['cand'] / plan['cand_group'] need one row per scene")
        K = max([len(r) for r in cand_rows] + [0])
        if K > MAX_CANDIDATES:
            raise ValueError("more than %d candidates in one scene" % MAX_CANDIDATES)
        cand = np.full((B, K), -1, np.int32)
        grp = np.full((B, K), -1, np.int32)
        dz = np.zeros((B, K), np.float64)
        paste = np.zeros(B, np.int64)
        if self.use_road_plane and any(len(r) for r in cand_rows) and (road_planes is None or calib is None):
            raise ValueError("USE_ROAD_PLANE needs road_planes and calib")
        for b in range(B):
            r = np.asarray(cand_rows[b], np.int64).reshape(-1)
            g = np.asarray(grp_rows[b], np.int32).reshape(-1)
            if len(g) != len(r):
                raise ValueError("plan['cand_group'][%d] does not match plan['cand'][%d]" % (b, b))
            cand[b, :len(r)] = r
            grp[b, :len(r)] = g
            ok = (r >= 0) & (r < (db.n_obj if db is not None else 0))
            if len(r) and db is not None:
                paste[b] = int(db.sizes[r[ok]].sum())
                if self.use_road_plane:
                    dz[b, :len(r)][ok] = self._mv_height(r[ok], road_planes[b], calib[b])
        paste_cap = int(paste.max()) if B else 0
        n_cand = int((cand >= 0).sum())
        fx = np.asarray(plan.get('flip_x', np.zeros(B)), np.int32).reshape(B)
        fy = np.asarray(plan.get('flip_y', np.zeros(B)), np.int32).reshape(B)
        flip = np.ascontiguousarray(np.stack([fx, fy], 1).astype(np.int32))
        angle = np.asarray(plan.get('angle', np.zeros(B)), np.float64).reshape(B)
        scale = np.asarray(plan.get('scale', np.ones(B)), np.float32).reshape(B)

        # ---- one upload: plan | class column | host scenes --------------------------------------------------------------
        parts = [cand, grp, dz, flip, angle, scale, np.concatenate(cls_rows).astype(np.float32) if m_total else np.zeros(0, np.float32)]
        if not dev_in:
            parts += [offs_h, offsets_of([len(g) for g in bl]), packed,
                      np.concatenate(bl, 0) if m_total else np.zeros((0, 7), np.float32)]
        if self.program is not None:
            ops, scene_draws, box_draws, D = self._program_draws(plan, B, fx, fy, angle, scale)
            parts += [scene_draws, box_draws]
            if self.pyramid is not None:
                py = self._pyramid_draws(plan, B)
                parts += list(py[:5])
        views = upload(parts, dev, pinned=True)
        d_cand, d_grp, d_dz, d_flip, d_angle, d_scale, d_cls = views[:7]
        if not dev_in:
            offs, boffs, pts, bxs7 = views[7:11]
        bxs = torch.cat([bxs7.to(torch.float32), d_cls.view(-1, 1)], dim=1).contiguous()

        # ---- the launch ------------------------------------------------------------------------------------------------
        ws = workspace("pda_augment_workspace_bytes", (B, n_cap, K),
                       "batch %d / n_cap %d / %d candidates out of range" % (B, n_cap, K), dev)
        out_cap = n_total + int(paste.sum())
        box_cap = m_total + n_cand
        out = torch.empty((max(out_cap, 1), C), dtype=torch.float32, device=dev)
        out_boxes = torch.empty((max(box_cap, 1), 8), dtype=torch.float32, device=dev)
        out_offs = torch.empty((B + 1,), dtype=torch.int64, device=dev)
        out_boffs = torch.empty((B + 1,), dtype=torch.int64, device=dev)
        info = torch.empty((B, 4), dtype=torch.int32, device=dev)
        if db is not None:
            dbp = (db.points.data_ptr() if db.points.numel() else None, db.offsets.data_ptr(), db.points.shape[0],
                   db.boxes.data_ptr() if db.n_obj else None, db.centre.data_ptr() if db.n_obj else None,
                   db.classes.data_ptr() if db.n_obj else None, db.n_obj)
        else:
            dbp = (None, None, 0, None, None, None, 0)
        if self.program is not None:
            _call("pda_augment_paste", pts, _chk(pts, "points", F32) if n_total else None, _chk(offs, "offsets", torch.int64), n_total,
                  B, C, n_cap, bxs.data_ptr() if m_total else None, _chk(boffs, "box_offsets", torch.int64), m_total, *dbp,
                  d_cand.data_ptr() if K else None, d_grp.data_ptr() if K else None, d_dz.data_ptr() if K else None, K,
                  self._rew_c, paste_cap, out.data_ptr(), out_cap, out_offs.data_ptr(), out_boxes.data_ptr(), box_cap,
                  out_boffs.data_ptr(), info.data_ptr(), ws.data_ptr())
            # the pasted scenes through the ordered program
            n_ops = len(self.program)
            if self.pyramid is not None:             # the hold: class 0 and the headings stay for pda_pyramid_aug
                ops = np.concatenate([ops, np.array([[OP_HOLD, 0]], np.int32)], 0)
                n_ops += 1
            d_scene, d_box = views[11 if not dev_in else 7], views[12 if not dev_in else 8]
            slots = min(MAX_SCENE_BOXES, max([len(c) + int((cand[b] >= 0).sum()) for b, c in enumerate(cls_rows)] + [0]))
            ws2 = workspace("pda_augment_steps_workspace_bytes", (B, n_cap + paste_cap, slots, n_ops),
                            "batch %d / n_cap %d / %d ops out of range" % (B, n_cap + paste_cap, n_ops), dev)
            out2, out_boxes2 = torch.empty_like(out), torch.empty_like(out_boxes)
            out_offs2, out_boffs2, info2 = torch.empty_like(out_offs), torch.empty_like(out_boffs), torch.empty_like(info)
            _call("pda_augment_steps", out, out.data_ptr(), out_offs.data_ptr(), out_cap, B, C, n_cap + paste_cap,
                  out_boxes.data_ptr(), out_boffs.data_ptr(), box_cap, ops.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n_ops,
                  d_scene.data_ptr(), d_box.data_ptr(), D, slots, info.data_ptr(), out2.data_ptr(), out_cap,
                  out_offs2.data_ptr(), out_boxes2.data_ptr(), box_cap, out_boffs2.data_ptr(), info2.data_ptr(), ws2.data_ptr())
            if self.pyramid is not None:
                pr = self.pyramid
                ws3 = workspace("pda_pyramid_aug_workspace_bytes", (B, n_cap + paste_cap, slots),
                                "batch %d / n_cap %d / %d boxes out of range" % (B, n_cap + paste_cap, slots), dev)
                out3, out_boxes3 = torch.empty_like(out), torch.empty_like(out_boxes)
                out_offs3, out_boffs3, info3 = torch.empty_like(out_offs), torch.empty_like(out_boffs), torch.empty_like(info)
                d_f64, d_i32, d_key, d_keep, d_n = views[-5:]
                probs = (ctypes.c_double * 3)(pr['drop_prob'], pr['sparsify_prob'], pr['swap_prob'])
                _call("pda_pyramid_aug", out2, out2.data_ptr(), out_offs2.data_ptr(), out_cap, B, C, n_cap + paste_cap,
                      out_boxes2.data_ptr(), out_boffs2.data_ptr(), box_cap, d_f64.data_ptr(), d_i32.data_ptr(), d_key.data_ptr(),
                      d_keep.data_ptr() if d_keep.numel() else None, d_n.data_ptr(), py[5], probs,
                      pr['sparsify_max'], pr['swap_max'], slots, info2.data_ptr(), out3.data_ptr(), out_cap, out_offs3.data_ptr(),
                      out_boxes3.data_ptr(), box_cap, out_boffs3.data_ptr(), info3.data_ptr(), ws3.data_ptr())
                out2, out_offs2, out_boxes2, out_boffs2, info2 = out3, out_offs3, out_boxes3, out_boffs3, info3
            if check:
                raise_on_status(info2.cpu(), _RULES)
            return (out2, out_offs2, n_cap + paste_cap), (out_boxes2, out_boffs2), info2
        _call("pda_augment", pts, _chk(pts, "points", F32) if n_total else None, _chk(offs, "offsets", torch.int64), n_total, B, C,
              n_cap, bxs.data_ptr() if m_total else None, _chk(boffs, "box_offsets", torch.int64), m_total, *dbp,
              d_cand.data_ptr() if K else None, d_grp.data_ptr() if K else None, d_dz.data_ptr() if K else None, K,
              d_flip.data_ptr(), d_angle.data_ptr(), d_scale.data_ptr(), self._rew_c, paste_cap, out.data_ptr(), out_cap,
              out_offs.data_ptr(), out_boxes.data_ptr(), box_cap, out_boffs.data_ptr(), info.data_ptr(), ws.data_ptr())
        if check:
            raise_on_status(info.cpu(), _RULES)
        return (out, out_offs, n_cap + paste_cap), (out_boxes, out_boffs), info


def from_config(cfg, database=None):
    """DataAugmentor of a loaded yaml (pdanet_amd.config.load_yaml): DATA_CONFIG.DATA_AUGMENTOR and CLASS_NAMES."""
    return DataAugmentor(cfg['DATA_CONFIG']['DATA_AUGMENTOR'], cfg['CLASS_NAMES'], database)
