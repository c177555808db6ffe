"""The anchor heads of the nuScenes yamls -- ResidualCoder with encode_angle_by_sincos and velocity columns, WeightedL1Loss,
9-column boxes through the multi-class NMS, and the two detectors of nuscenes_multihead.py -- against
tests/golden/anchor_head_coded.npz: the reference's own AnchorHeadMulti, assigner, coder, losses and post_processing on CPU
tensors (tests/golden/make_anchor_head_coded_golden.py).

CPU part: the symbols, argument validation before any HIP call, the refusals (the new ones, and that AnchorHeadMulti still
refuses), state-dict keys and anchors, both detectors from the yamls' MODEL blocks, and the float64 restatement
(tests/golden/anchor_head_coded_restatement.py) against the fixture.  GPU part: the kernels against the fixture and the
restatement, and bit for bit against the 7-column entries on tests/golden/anchor_head_multi.npz.

Tolerances.  Labels, weights and counts equal.  Target columns 0-2, the scalar heading and the velocity columns bit-identical,
NaN at the same places; the log columns within one float32 ulp (tests/test_anchor_head.py).  The sincos columns within 2^-22
absolute: the reference's float32 cosine and sine are each within 1 ulp (at most 2^-24 for values in [-1, 1]) of the
once-rounded value, two operands, plus the rounding of a difference below 2 (half an ulp of at most 2^-23); the kernels against
the restatement bit for bit.  Losses within LOSS_TOL = 2e-5 on the terms, gradients within 2e-5 of the largest reference
gradient.  Decoded sincos headings within 2^-22 / min_hypot + 2 ulp(pi): the atan2's arguments are off by at most 2^-22 as
above, its derivative is at most 1 / hypot, min_hypot is recorded by the maker, and the result (at most pi) is rounded once on
each side.  Sizes within 2 ulp, headings behind the direction classifier within 2 ulp, velocities bit-identical."""
import ctypes
import gc
import json
import os
import sys

import numpy as np
import pytest
import torch

from pdanet_amd import _lib, anchor_head as ah, anchor_head_coded as ahc, anchor_head_multi as ahm, build, model_nms_utils
from pdanet_amd import nuscenes_multihead
from pdanet_amd.config import to_attr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import anchor_head_coded_restatement as crs  # noqa: E402
import test_anchor_head_multi as tm  # noqa: E402
from test_anchor_head import LOSS_TOL, bits_equal, ulps  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "anchor_head_coded.npz")
G = np.load(FIXTURE)
SETUP = json.loads(str(G['configs']))
CONFIGS, POST, CLASS_NAMES, LAYOUT = SETUP['heads'], SETUP['post'], SETUP['class_names'], SETUP['layout']
with open(os.path.join(HERE, "golden", "anchor_head_coded_state_dicts.json")) as _f:
    STATE = json.load(_f)
B = 2
BATCHES = [(c, t) for c in 'nsv' for t in 'xyz']
KEYS = ['rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir', 'rpn_loss']
SINCOS_TOL = 2.0 ** -22
PI_ULP = float(np.spacing(np.float32(np.pi)))


def make_head(c, input_channels=16, cls=ahc.AnchorHeadMultiCoded, **over):
    pcr, vs = np.array(SETUP['point_cloud_range'], np.float64), np.array(SETUP['voxel_size'], np.float64)
    grid = np.round((pcr[3:] - pcr[:3]) / vs).astype(np.int64)
    head_cfg = json.loads(json.dumps(CONFIGS[c]))
    for path, value in over.items():
        node = head_cfg
        keys = path.split('__')
        for k in keys[:-1]:
            node = node[k]
        if value is None:
            node.pop(keys[-1], None)
        else:
            node[keys[-1]] = value
    return cls(model_cfg=to_attr(head_cfg), input_channels=input_channels, num_class=len(CLASS_NAMES[c]), class_names=CLASS_NAMES[c],
               grid_size=grid, point_cloud_range=pcr, predict_boxes_when_training=False)


def class_arrays(c):
    gen = CONFIGS[c]['ANCHOR_GENERATOR_CONFIG']
    return ([CLASS_NAMES[c].index(g['class_name']) + 1 for g in gen], [g['matched_threshold'] for g in gen],
            [g['unmatched_threshold'] for g in gen], [int(v) for v in G[c + '_class_rows']])


def layout(c):
    """Per prediction tensor of the loss: its rows, logit columns and column base (one tensor when not separate)."""
    class_rows = [int(v) for v in G[c + '_class_rows']]
    if not CONFIGS[c]['SEPARATE_MULTIHEAD']:
        return [sum(class_rows)], [len(CLASS_NAMES[c])], [0]
    rows, cols, at = [], [], 0
    for h in CONFIGS[c]['RPN_HEAD_CFGS']:
        k = len(h['HEAD_CLS_NAME'])
        rows.append(sum(class_rows[at:at + k]))
        cols.append(k)
        at += k
    return rows, cols, [sum(cols[:h]) for h in range(len(cols))]


def preds_of(c):
    """The per-tensor lists (cls, box, dir | None) of configuration c."""
    rows, cols, bases = layout(c)
    out = []
    for i, k in enumerate(('cls', 'box', 'dir')):
        key = '%s_%s_preds' % (c, k)
        if key not in G:
            out.append(None)
            continue
        x, parts, at = G[key].astype(np.float32), [], 0
        for h, n in enumerate(rows):
            part = x[:, at:at + n]
            if i == 0 and len(rows) > 1:
                part = part[..., bases[h]:bases[h] + cols[h]]
            parts.append(np.ascontiguousarray(part))
            at += n
        out.append(parts)
    return out


def same_with_nan(a, b):
    """Bit-identical where b is a number, NaN where b is NaN."""
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and bits_equal(np.where(nan, 0, a), np.where(nan, 0, b))


def check_targets(c, t, labels, targets, weights, num_pos):
    p = c + t + '_'
    code, sincos, extra = LAYOUT[c]
    ref_l, ref_t, ref_w = G[p + 'box_cls_labels'], G[p + 'box_reg_targets'], G[p + 'reg_weights']
    assert labels.dtype == np.int32 and labels.shape == ref_l.shape and targets.shape == ref_t.shape == ref_l.shape + (code,)
    assert np.array_equal(labels, ref_l), "labels"
    assert bits_equal(weights, ref_w), "reg_weights"
    assert np.array_equal(num_pos, (ref_l > 0).sum(axis=1)), "num_pos"
    assert bits_equal(targets[..., :3], ref_t[..., :3]), "centre targets"
    d = ulps(targets[..., 3:6], ref_t[..., 3:6])
    assert d.max() <= 1, "log targets"
    if sincos:
        err = float(np.abs(targets[..., 6:8].astype(np.float64) - ref_t[..., 6:8]).max())
        print("targets", c, t, "sincos columns off by %.3g (bound %.3g)" % (err, SINCOS_TOL))
        assert err <= SINCOS_TOL, "sincos targets"
    else:
        assert bits_equal(targets[..., 6], ref_t[..., 6]), "heading targets"
    if extra:
        assert same_with_nan(targets[..., code - extra:], ref_t[..., code - extra:]), "velocity targets"
    assert not np.isnan(targets[..., :code - extra]).any()


def loss_kwargs(c):
    cfg = CONFIGS[c]
    w = cfg['LOSS_CONFIG']['LOSS_WEIGHTS']
    has_dir = bool(cfg.get('USE_DIRECTION_CLASSIFIER'))
    return dict(num_class=len(CLASS_NAMES[c]), code_weights=w['code_weights'], cls_weight=w['cls_weight'], loc_weight=w['loc_weight'],
                dir_weight=w['dir_weight'] if has_dir else 0.0, dir_offset=cfg['DIR_OFFSET'] if has_dir else 0.0,
                pos_cls_weight=w.get('pos_cls_weight', 1.0), neg_cls_weight=w.get('neg_cls_weight', 1.0), sincos=LAYOUT[c][1])


def check_losses(c, t, terms, grads):
    """terms: the four loss terms; grads: (cls, box, dir | None) lists of per-tensor gradients."""
    p = c + t + '_'
    d_loss = np.abs(np.asarray(terms, np.float64) - G[p + 'losses'])
    refs, got = [], []
    for name, parts in zip(('cls', 'box', 'dir'), grads):
        for h, v in enumerate(parts or []):
            refs.append(G['%sg_%s_%d' % (p, name, h)])
            got.append(np.asarray(v, np.float64).reshape(refs[-1].shape))
    scale = max(float(np.abs(v).max()) for v in refs)
    d_g = max(float(np.abs(g - r).max()) for g, r in zip(got, refs))
    print("loss", c, t, "terms", ["%.3g" % v for v in d_loss], "grad %.3g of %.3g" % (d_g, scale))
    assert d_loss.max() <= LOSS_TOL
    assert d_g <= LOSS_TOL * scale
    return got


def check_decode(c, boxes):
    code, sincos, extra = LAYOUT[c]
    ref = G[c + '_batch_box_preds']
    assert boxes.shape == ref.shape == (B, len(G[c + '_table']), 7 + extra)
    assert bits_equal(boxes[..., :3], ref[..., :3]), "centres"
    assert ulps(boxes[..., 3:6], ref[..., 3:6]).max() <= 2, "sizes"
    if sincos:
        bound = SINCOS_TOL / float(G[c + '_min_hypot']) + 2 * PI_ULP
        err = float(np.abs(boxes[..., 6].astype(np.float64) - ref[..., 6]).max())
        print("decode", c, "headings off by %.3g (bound %.3g)" % (err, bound))
        assert err <= bound, "sincos heading"
    else:
        assert ulps(boxes[..., 6], ref[..., 6]).max() <= 2, "heading behind the direction classifier"
    if extra:
        assert bits_equal(boxes[..., 7:], ref[..., 7:]), "velocities"


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


NAMES = ["pda_anchor_assign_targets_coded", "pda_anchor_multi_assign_targets_coded", "pda_anchor_loss_coded",
         "pda_anchor_multi_loss_coded", "pda_anchor_decode_coded", "pda_multi_nms_compact_wide"]


def test_symbols_exported(lib):
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.pda_abi_version() == 20


def test_fixture_is_small_and_covers_the_cases():
    assert os.path.getsize(FIXTURE) < 1 << 20
    assert LAYOUT == {'n': [10, 1, 2], 's': [8, 1, 0], 'v': [9, 0, 2]}
    assert G['n_table'].shape == (990, 7) and G['s_table'].shape == (891, 7) and G['v_table'].shape == (891, 7)
    assert layout('n') == ([198, 396, 396], [1, 2, 2], [0, 1, 3]) and layout('s') == ([891], [3], [0])
    assert 'n_dir_preds' not in G and 's_dir_preds' not in G and 'v_dir_preds' in G
    for c in 'nsv':
        code, sincos, extra = LAYOUT[c]
        assert all(int(r) % 64 for r in G[c + '_class_rows']) and len(G[c + '_table']) % 64 and len(G[c + '_table']) % 256
        gt = G[c + 'x_gt_boxes'][0]
        assert gt.shape == (12, 8 + extra) and bits_equal(gt[0], gt[1])
        zero = ~(np.nan_to_num(gt, nan=1.0) != 0).any(axis=1)
        assert zero[6] and not zero[7] and zero[-3:].all()
        labels, targets = G[c + 'x_box_cls_labels'], G[c + 'x_box_reg_targets']
        assert targets.shape[-1] == code and (labels[0] < 0).any() and (G[c + 'z_box_cls_labels'] == 0).all()
        if extra:
            nan = np.isnan(targets[labels > 0][:, code - extra:])
            assert nan.any(axis=1).sum() >= 2 and (nan.sum(axis=1) == 1).any()      # NaN velocities, one in one column only
        if sincos:
            assert float(G[c + '_min_hypot']) >= 0.25
    b, n, col = (int(v) for v in G['n_kink'])                                        # the kink of the L1 term
    assert G['nx_box_cls_labels'][b, n] > 0 and G['n_box_preds'].astype(np.float32)[b, n, col] == G['nx_box_reg_targets'][b, n, col]
    assert CONFIGS['n']['LOSS_CONFIG']['REG_LOSS_TYPE'] == 'WeightedL1Loss'
    assert CONFIGS['n']['LOSS_CONFIG']['LOSS_WEIGHTS']['code_weights'] == [1.0] * 8 + [0.2] * 2
    pre, post = POST['NMS_CONFIG']['NMS_PRE_MAXSIZE'], POST['NMS_CONFIG']['NMS_POST_MAXSIZE']
    rows, cols, _ = layout('n')
    thr = np.log(POST['SCORE_THRESH'] / (1 - POST['SCORE_THRESH']))
    above = [(G['post_n_cls_%d' % h] >= thr).sum(axis=1) for h in range(len(rows))]
    assert min(rows) > pre and max(int(a.max()) for a in above) > pre and min(int(a.min()) for a in above) == 0
    counts = [np.bincount(G['post_n_pred_labels'][s, :G['post_n_num_pred'][s]], minlength=6) for s in range(B)]
    assert max(int(v.max()) for v in counts) == post and counts[1][5] == 0 and counts[0][5] > 0
    assert G['post_n_pred_boxes'].shape[-1] == 9 and G['post_n_boxes'].shape == (B, 990, 9)


def test_argument_validation_without_gpu(lib):
    d = ctypes.c_double
    lab = (ctypes.c_int32 * 2)(1, 2)
    thr = (ctypes.c_float * 2)(0.6, 0.5)
    rows = (ctypes.c_int32 * 2)(5, 3)
    for name in ("pda_anchor_assign_targets_coded", "pda_anchor_multi_assign_targets_coded"):
        count = rows if 'multi' in name else (ctypes.c_int32 * 2)(1, 1)
        assign = lambda cols, sincos, b=1, m=4, n=8, n_cls=2: getattr(lib, name)(
            None, cols, sincos, b, m, None, n, n_cls, lab, thr, thr, count, None, None, None, None, None, None)
        for cols in (7, 11, 0, -1):
            assert assign(cols, 0) == 1 and b"gt_cols" in lib.pda_last_error()
        for sincos in (2, -1):
            assert assign(10, sincos) == 1 and b"sincos" in lib.pda_last_error()
        assert assign(10, 1, n_cls=0) == 1 and b"n_cls" in lib.pda_last_error()
        assert assign(10, 1, b=0) == 0 and assign(8, 0, b=0) == 0 and assign(9, 1, b=0) == 0      # the empty problem
        for cols in (8, 9, 10):
            assert assign(cols, 1) == 1 and b"null" in lib.pda_last_error()
    w = (ctypes.c_float * 10)(*[1.0] * 10)
    one = ctypes.c_void_p(8)      # a non-null pointer that a rejected call never reads
    single = lambda code, sincos, reg, dirs=None, b=1: lib.pda_anchor_loss_coded(
        code, sincos, reg, None, None, dirs, None, None, None, None, b, 8, 3, 2, w, d(1), d(2), d(0.2), d(0.78), None, None, None, None,
        None, None)
    ptrs = (ctypes.c_void_p * 2)(None, None)
    cols, base = (ctypes.c_int32 * 2)(1, 2), (ctypes.c_int32 * 2)(0, 1)
    multi = lambda code, sincos, reg, dirs=None, heads=2, b=1: lib.pda_anchor_multi_loss_coded(
        code, sincos, reg, ptrs, ptrs, dirs, heads, rows, cols, base, None, None, None, None, b, 8, 3, 2, w, d(1), d(2), d(0.2),
        d(0.78), d(1), d(1), ptrs, ptrs, ptrs, None, None, None)
    decode = lambda code, sincos, reg=0, dirs=None, b=1: lib.pda_anchor_decode_coded(code, sincos, None, dirs, None, b, 8, 2, d(0.78),
                                                                                     d(0), None, None)
    for fn, dirs in ((single, one), (multi, ptrs), (decode, one)):
        for code, sincos in ((6, 0), (10, 0), (7, 1), (11, 1), (0, 0), (-3, 1)):
            assert fn(code, sincos, 0) == 1 and b"code=" in lib.pda_last_error()
        for sincos in (2, -1):
            assert fn(9, sincos, 0) == 1 and b"sincos" in lib.pda_last_error()
        for code in (8, 9, 10):
            assert fn(code, 1, 0, dirs=dirs) == 1 and b"sincos with dir_cls_preds" in lib.pda_last_error()
    for fn in (single, multi):
        for reg in (2, -1):
            assert fn(10, 1, reg) == 1 and b"reg_loss" in lib.pda_last_error()
        assert fn(10, 1, 1, b=0) == 1
    assert single(10, 1, 1) == 1 and b"null pointer" in lib.pda_last_error()
    assert single(9, 0, 0, dirs=one) == 1 and b"null pointer" in lib.pda_last_error()
    assert multi(10, 1, 1, heads=0) == 1 and b"n_heads" in lib.pda_last_error()
    assert multi(10, 1, 1, heads=33) == 1 and b"n_heads" in lib.pda_last_error()
    assert multi(10, 1, 1) == 1 and b"null pointer of head 0" in lib.pda_last_error()
    assert decode(10, 1) == 1 and b"null pointer" in lib.pda_last_error() and decode(10, 1, b=0) == 0
    compact = lambda width, b=1, c=3, k=8, post=4: lib.pda_multi_nms_compact_wide(width, None, None, None, None, None, b, c, k, post,
                                                                                 None, None, None, None, None)
    for width in (6, 10, 0):
        assert compact(width) == 1 and b"box_cols" in lib.pda_last_error()
    assert compact(9, c=0) == 1 and b"problems" in lib.pda_last_error() and compact(9, c=257) == 1
    assert compact(9, b=0) == 0 and compact(9) == 1 and b"null" in lib.pda_last_error()


def test_new_refusals():
    for over in ({'TARGET_ASSIGNER_CONFIG__POS_FRACTION': 0.5}, {'TARGET_ASSIGNER_CONFIG__NORM_BY_NUM_EXAMPLES': True},
                 {'TARGET_ASSIGNER_CONFIG__MATCH_HEIGHT': True}, {'TARGET_ASSIGNER_CONFIG__NAME': 'ATSS'}, {'USE_MULTIHEAD': False},
                 {'USE_DIRECTION_CLASSIFIER': True}, {'LOSS_CONFIG__REG_LOSS_TYPE': 'WeightedL2Loss'},
                 {'TARGET_ASSIGNER_CONFIG__BOX_CODER_CONFIG': {'code_size': 10, 'encode_angle_by_sincos': True}},
                 {'TARGET_ASSIGNER_CONFIG__BOX_CODER_CONFIG': {'code_size': 6}}):
        with pytest.raises(NotImplementedError):
            make_head('n', **over)
    gen = json.loads(json.dumps(CONFIGS['n']['ANCHOR_GENERATOR_CONFIG']))
    gen[1]['anchor_bottom_heights'] = [-1.6, -0.6]
    with pytest.raises(NotImplementedError, match="bottom height"):
        make_head('n', ANCHOR_GENERATOR_CONFIG=gen)
    with pytest.raises(ValueError, match="code_weights"):
        make_head('n', LOSS_CONFIG__LOSS_WEIGHTS__code_weights=[1.0] * 7)
    with pytest.raises(NotImplementedError, match="USE_MULTIHEAD"):
        make_head('n', cls=ahc.AnchorHeadSingleCoded, RPN_HEAD_CFGS=None)
    head = make_head('n')
    for cols in (8, 9, 11):
        with pytest.raises(ValueError, match="gt_boxes"):
            head.target_assigner.assign_targets(head.anchors, torch.zeros(1, 4, cols))
    with pytest.raises(ValueError, match="gt_boxes"):
        make_head('s').target_assigner.assign_targets(head.anchors, torch.zeros(1, 4, 10))
    with pytest.raises(RuntimeError, match="no CPU path"):
        head.assign_targets(torch.zeros(1, 4, 10))
    cls, box, _ = ([torch.from_numpy(v) for v in parts] if parts else None for parts in preds_of('n'))
    args = ([1, 2, 2], [0, 1, 3], torch.from_numpy(G['nx_box_cls_labels']), torch.from_numpy(G['nx_box_reg_targets']),
            torch.zeros(2, dtype=torch.int32), torch.from_numpy(G['n_table']), 5)
    with pytest.raises(NotImplementedError, match="direction classifier"):
        ahc.anchor_multi_loss_coded(cls, box, cls, *args, [1.0] * 10, 1.0, 2.0, sincos=1)
    with pytest.raises(ValueError, match="code weights"):
        ahc.anchor_multi_loss_coded(cls, box, None, *args, [1.0] * 9, 1.0, 2.0, sincos=1)
    with pytest.raises(NotImplementedError, match="REG_LOSS_TYPE"):
        ahc.anchor_multi_loss_coded(cls, box, None, *args, [1.0] * 10, 1.0, 2.0, sincos=1, reg_loss='Huber')
    with pytest.raises(RuntimeError, match="no CPU path"):
        ahc.anchor_multi_loss_coded(cls, box, None, *args, [1.0] * 10, 1.0, 2.0, sincos=1, reg_loss='WeightedL1Loss')
    with pytest.raises(NotImplementedError, match="columns"):
        model_nms_utils.multi_classes_nms_batched([torch.zeros(1, 4, 1)], torch.zeros(1, 4, 10), [torch.tensor([1])], POST['NMS_CONFIG'], 0.1)


def test_the_old_classes_still_refuse():
    for c in 'nsv':
        with pytest.raises(NotImplementedError):
            make_head(c, cls=ahm.AnchorHeadMulti)
    plain = tm.make_head('a')
    with pytest.raises(NotImplementedError, match="7 \\+ 1"):
        plain.target_assigner.assign_targets(plain.anchors, torch.zeros(1, 4, 10))
    coder = make_head('n').box_coder
    with pytest.raises(NotImplementedError):
        ahm.ClassMajorTargetAssigner(to_attr(CONFIGS['n']), CLASS_NAMES['n'], coder)
    with pytest.raises(NotImplementedError, match="7 columns"):
        ahm.anchor_multi_loss([torch.zeros(1, 4, 1)], [torch.zeros(1, 4, 10)], None, [1], [0], torch.zeros(1, 4, dtype=torch.int32),
                              torch.zeros(1, 4, 10), torch.zeros(1, dtype=torch.int32), torch.zeros(4, 7), 1, [1.0] * 10, 1.0, 1.0)


def test_state_dict_keys_and_anchors_are_the_references():
    for c in 'nsv':
        head = make_head(c)
        sd = head.state_dict()
        assert list(sd.keys()) == [str(k) for k in G['keys_' + c]]
        assert [list(v.shape) for v in sd.values()] == json.loads(str(G['shapes_' + c]))
        head.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
        for i, a in enumerate(head.anchors):
            assert bits_equal(a.numpy(), G['%s_anchors_%d' % (c, i)]), "anchors of class %d" % i
        table, class_rows = ahm.class_major_table(head.anchors)
        assert bits_equal(table.numpy(), G[c + '_table']) and class_rows == [int(v) for v in G[c + '_class_rows']]
        assert head.box_coder.code_size == LAYOUT[c][0] and ahc.code_layout(head.box_coder) == tuple(LAYOUT[c])
    n = make_head('n')
    assert [[k, list(v.shape)] for k, v in n.state_dict().items()] == STATE['head_n']
    assert [h.num_class for h in n.rpn_heads] == [1, 2, 2] and n.shared_conv is not None and n.rpn_heads[0].conv_dir_cls is None
    assert list(n.rpn_heads[0].conv_box.keys()) == ['conv_reg', 'conv_height', 'conv_size', 'conv_angle', 'conv_velo']
    assert type(n.reg_loss_func).__name__ == 'WeightedL1Loss' and type(make_head('s').reg_loss_func).__name__ == 'WeightedSmoothL1Loss'


def dataset_of(name):
    return STATE[name]['config']['dataset']


@pytest.mark.parametrize("name", ["PointPillar", "SECONDNet"])
def test_detectors_build_from_the_yamls(name):
    cfg = STATE[name]['config']
    head_cfg = cfg['MODEL']['DENSE_HEAD']
    assert cfg['MODEL']['NAME'] == name and head_cfg['NAME'] == 'AnchorHeadMulti' and head_cfg['LOSS_CONFIG']['REG_LOSS_TYPE'] == 'WeightedL1Loss'
    assert head_cfg['TARGET_ASSIGNER_CONFIG']['BOX_CODER_CONFIG'] == {'code_size': 9, 'encode_angle_by_sincos': True}
    model = nuscenes_multihead.build(to_attr(cfg['MODEL']), 10, dataset_of(name))
    children = ['vfe', 'map_to_bev_module', 'backbone_2d', 'dense_head'] if name == 'PointPillar' else \
        ['vfe', 'backbone_3d', 'map_to_bev_module', 'backbone_2d', 'dense_head']
    assert [n for n, _ in model.named_children()] == children
    assert type(model) is nuscenes_multihead.DETECTORS[name] and isinstance(model.dense_head, ahc.AnchorHeadMultiCoded)
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == STATE[name]['state_dict']
    assert len(model.dense_head.rpn_heads) == 6 and model.dense_head.box_coder.code_size == 10
    with pytest.raises(NotImplementedError, match="NAME"):
        nuscenes_multihead.build(to_attr(dict(cfg['MODEL'], NAME='PVRCNN')), 10, dataset_of(name))


@pytest.mark.parametrize("c,t", BATCHES)
def test_restatement_targets(c, t):
    check_targets(c, t, *crs.assign_targets(G[c + t + '_gt_boxes'], G[c + '_table'], *class_arrays(c), LAYOUT[c][1]))


@pytest.mark.parametrize("c,t", BATCHES)
def test_restatement_losses_and_gradients(c, t):
    p = c + t + '_'
    cls, box, d = preds_of(c)
    _, cols, bases = layout(c)
    terms, grads = crs.losses(cls, box, d, cols, bases, G[p + 'box_cls_labels'], G[p + 'box_reg_targets'], G[c + '_table'],
                              l1=CONFIGS[c]['LOSS_CONFIG'].get('REG_LOSS_TYPE') == 'WeightedL1Loss', **loss_kwargs(c))
    check_losses(c, t, terms, grads)


@pytest.mark.parametrize("c", "nsv")
def test_restatement_decode(c):
    cfg = CONFIGS[c]
    d = G[c + '_dir_preds'].astype(np.float32) if c + '_dir_preds' in G else None
    check_decode(c, crs.decode(G[c + '_box_preds'].astype(np.float32), d, G[c + '_table'], cfg.get('DIR_OFFSET', 0.0) if d is not None else 0.0,
                               cfg.get('DIR_LIMIT_OFFSET', 0.0) if d is not None else 0.0, sincos=LAYOUT[c][1]))


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run_targets(head, gt):
    ret = head.assign_targets(gt)
    return ret, tuple(ret[k].cpu().numpy() for k in ('box_cls_labels', 'box_reg_targets', 'reg_weights', 'num_pos'))


@gpu
@pytest.mark.parametrize("c,t", BATCHES)
def test_gpu_targets(c, t):
    head = make_head(c).cuda()
    gt = dev(G[c + t + '_gt_boxes'])
    before = gt.clone()
    _, got = run_targets(head, gt)
    check_targets(c, t, *got)
    assert same_with_nan(gt.cpu().numpy(), before.cpu().numpy()), "gt_boxes was written"
    ref = crs.assign_targets(G[c + t + '_gt_boxes'], G[c + '_table'], *class_arrays(c), LAYOUT[c][1])
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[3], ref[3])
    if LAYOUT[c][1]:
        assert bits_equal(got[1][..., 6:8], ref[1][..., 6:8]), "sincos columns against the restatement"


@gpu
@pytest.mark.parametrize("t", "xyz")
def test_gpu_slot_major_targets_equal_the_class_major_ones_permuted(t):
    """Configuration n's classes share stride and rotations, so its anchors also form a location-major table: the slot-major
    entry on that table gives the class-major targets, row for row."""
    single = make_head('n', cls=ahc.AnchorHeadSingleCoded, USE_MULTIHEAD=None, SEPARATE_MULTIHEAD=None, RPN_HEAD_CFGS=None,
                       SHARED_CONV_NUM_FILTER=None, SEPARATE_REG_CONFIG=None)
    ny, nx = single.anchors[0].shape[1:3]
    c, a, y, x = np.meshgrid(np.arange(5), np.arange(2), np.arange(ny), np.arange(nx), indexing='ij')
    perm = (((y * nx + x) * 5 + c) * 2 + a).reshape(-1)                  # class-major row i == location-major row perm[i]
    assert bits_equal(ah.anchor_table(single.anchors)[0].numpy()[perm], G['n_table'])
    gt = dev(G['n' + t + '_gt_boxes'])
    _, got = run_targets(make_head('n').cuda(), gt)
    _, ref = run_targets(single.cuda(), gt)
    check_targets('n', t, ref[0][:, perm], ref[1][:, perm], ref[2][:, perm], ref[3])
    assert np.array_equal(got[0], ref[0][:, perm]) and bits_equal(got[2], ref[2][:, perm]) and np.array_equal(got[3], ref[3])
    assert same_with_nan(got[1], ref[1][:, perm])


def head_loss(head, c, t):
    leaves = [None if parts is None else [dev(v).requires_grad_(True) for v in parts] for parts in preds_of(c)]
    one = (lambda v: v) if CONFIGS[c]['SEPARATE_MULTIHEAD'] else (lambda v: v[0])
    head.forward_ret_dict = dict({'cls_preds': one(leaves[0]), 'box_preds': one(leaves[1])},
                                 **head.assign_targets(dev(G[c + t + '_gt_boxes'])))
    if leaves[2] is not None:
        head.forward_ret_dict['dir_cls_preds'] = one(leaves[2])
    loss, tb = head.get_loss()
    return loss, tb, leaves


@gpu
@pytest.mark.parametrize("c,t", BATCHES)
def test_gpu_losses(c, t):
    code, sincos, extra = LAYOUT[c]
    head = make_head(c).cuda()
    loss, tb, leaves = head_loss(head, c, t)
    loss.backward()
    has_dir = leaves[2] is not None
    assert list(tb) == (KEYS if has_dir else [k for k in KEYS if k != 'rpn_loss_dir'])
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 and v.is_cuda for v in tb.values())
    terms = [float(tb[k]) if k in tb else 0.0 for k in KEYS]
    check_losses(c, t, terms, [None if parts is None else [v.grad.cpu().numpy() for v in parts] for parts in leaves])
    assert float(loss.detach()) == float(tb['rpn_loss'])
    g_box = np.concatenate([v.grad.cpu().numpy() for v in leaves[1]], axis=1)
    targets, labels = G[c + t + '_box_reg_targets'], G[c + t + '_box_cls_labels']
    assert np.isfinite(g_box).all() and not g_box[np.isnan(targets)].any(), "the gradient at a NaN target"
    assert not g_box[labels <= 0].any()
    if c == 'n' and t == 'x':
        b, n, col = (int(v) for v in G['n_kink'])
        assert g_box[b, n, col] == 0 and g_box[b, n, :8].all(), "the gradient at the kink of the L1 term"


@gpu
@pytest.mark.parametrize("c,t", tm.BATCHES)
def test_gpu_coded_entries_equal_the_seven_column_ones_bit_for_bit(c, t):
    """The coded entries at extra = 0, no sincos, smooth L1 on the batches of tests/golden/anchor_head_multi.npz: targets, the
    four loss terms and every gradient are the bits of the entries they were generalised from."""
    old = tm.make_head(c).cuda()
    new = tm.make_head(c, cls=ahc.AnchorHeadMultiCoded).cuda()
    gt = dev(tm.G[c + t + '_gt_boxes'])
    _, ref = run_targets(old, gt)
    _, got = run_targets(new, gt)
    for x, y in zip(got, ref):
        assert bits_equal(x, y)
    results = []
    for head in (old, new):
        loss, tb, leaves = tm.head_loss(head, c, t)
        loss.backward()
        results.append(([tb[k].cpu().numpy() for k in tb], [v.grad.cpu().numpy() for parts in leaves if parts is not None for v in parts]))
    assert len(results[0][0]) == len(results[1][0]) and len(results[0][1]) == len(results[1][1])
    for x, y in zip(results[0][0] + results[0][1], results[1][0] + results[1][1]):
        assert bits_equal(x, y)
    if t == 'x':      # the single-tensor loss and the decode
        cls, box, d = ([dev(v) for v in parts] if parts is not None else None for parts in tm.preds_of(c))
        join = lambda parts: None if parts is None else torch.cat(parts, dim=1)
        table = old.anchor_table(gt.device)
        assert bits_equal(ahc.anchor_decode_coded(join(box), join(d), table, 0.78539, 0.0).cpu().numpy(),
                          ah.anchor_decode(join(box), join(d), table, 0.78539, 0.0).cpu().numpy())
        if len(cls) == 1:
            args = (dev(tm.G[c + t + '_box_cls_labels']), dev(tm.G[c + t + '_box_reg_targets']), dev(ref[3]), table, 3, [1.0, 1.0, 0.5, 1.0, 1.0, 2.0, 0.75],
                    1.0, 2.0)
            outs = []
            for fn in (ah.anchor_loss, ahc.anchor_loss_coded):
                leaves = [cls[0].clone().requires_grad_(True), box[0].clone().requires_grad_(True)]
                loss, out = fn(leaves[0], leaves[1], None, *args)
                loss.backward()
                outs.append([out.cpu().numpy()] + [v.grad.cpu().numpy() for v in leaves])
            for x, y in zip(*outs):
                assert bits_equal(x, y)


def loss_case(n):
    """One scene of n anchors with 10-wide sincos codes under WeightedL1Loss: a head of one logit column over the first third of
    the rows and one of two columns over the rest (one head when n == 1), about 5 % ignored anchors, up to five positives (the
    first and the last anchor among them), one with a NaN velocity target and one whose prediction equals its target."""
    rng = np.random.default_rng(n)
    rows = [n] if n == 1 else [n // 3, n - n // 3]
    cols, bases = ([1], [0]) if n == 1 else ([1, 2], [0, 1])
    table = np.zeros((n, 7), np.float32)
    table[:, :2] = rng.uniform(-40, 40, (n, 2))
    table[:, 3:6] = (3.9, 1.6, 1.56)
    table[:, 6] = rng.choice(np.array([0.0, 1.57], np.float32), n)
    cls = [rng.normal(-4.0, 1.0, (1, r, k)).astype(np.float32) for r, k in zip(rows, cols)]
    box = [rng.normal(0.0, 0.3, (1, r, 10)).astype(np.float32) for r in rows]
    labels = np.where(rng.random((1, n)) < 0.05, -1, 0).astype(np.int32)
    pos = np.unique(np.linspace(0, n - 1, min(n, 5)).astype(np.int64))
    labels[0, pos] = np.where(pos < rows[0], 1, 2 + (pos % 2)).astype(np.int32)
    targets = np.zeros((1, n, 10), np.float32)
    targets[0, pos] = rng.normal(0.0, 0.3, (len(pos), 10))
    targets[0, pos[0], 8] = np.nan
    targets[0, pos[-1], 3] = box[-1][0, -1, 3]
    return cls, box, cols, bases, labels, targets, np.array([len(pos)], np.int32), table


LOSS_CASE_WEIGHTS = dict(num_class=3, code_weights=[1.0] * 8 + [0.2] * 2, cls_weight=1.0, loc_weight=0.25, pos_cls_weight=1.0,
                         neg_cls_weight=2.0, sincos=1)


@gpu
@pytest.mark.parametrize("n,blocks", [(1, 1), (1024, 1), (1025, 2), (1500, 2)])
def test_gpu_coded_multi_loss_at_the_block_boundaries(n, blocks):
    """10-wide rows at the sizes where the shared partial sums can go wrong: one anchor; exactly one workgroup of 1024; one
    anchor more; 1500, where the second head's rows (500..1499) straddle the two workgroups.  Against the float64 restatement,
    within test_gpu_losses' bound."""
    assert _lib.load().pda_anchor_multi_loss_blocks(n) == blocks
    cls, box, cols, bases, labels, targets, num_pos, table = loss_case(n)
    ref, ref_grads = crs.losses(cls, box, None, cols, bases, labels, targets, table, l1=True, **LOSS_CASE_WEIGHTS)
    leaves = [[dev(v).requires_grad_(True) for v in parts] for parts in (cls, box)]
    loss, out = ahc.anchor_multi_loss_coded(leaves[0], leaves[1], None, cols, bases, dev(labels), dev(targets), dev(num_pos), dev(table),
                                            reg_loss='WeightedL1Loss', **LOSS_CASE_WEIGHTS)
    loss.backward()
    d_loss = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    scale = max(float(np.abs(g).max()) for parts in ref_grads[:2] for g in parts)
    d_g = max(float(np.abs(v.grad.cpu().numpy() - g).max()) for parts, refs in zip(leaves, ref_grads[:2]) for v, g in zip(parts, refs))
    print("coded multi n", n, "losses", ref, "diff", ["%.3g" % v for v in d_loss], "grad %.3g of %.3g" % (d_g, scale))
    assert d_loss.max() <= LOSS_TOL and d_g <= LOSS_TOL * scale
    assert float(loss.detach()) == float(out[3])
    g_box = np.concatenate([v.grad.cpu().numpy() for v in leaves[1]], axis=1)
    assert np.isfinite(g_box).all() and g_box[0, 0, 8] == 0 and g_box[0, -1, 3] == 0      # the NaN target, the kink
    assert g_box[0, 0, [0, 1, 2, 4, 5, 6, 7, 9]].all() and not g_box[labels <= 0].any()


@gpu
@pytest.mark.parametrize("c", "nsv")
def test_gpu_decode(c):
    head = make_head(c).cuda().eval()
    cls, box, d = ([dev(v) for v in parts] if parts is not None else None for parts in preds_of(c))
    one = (lambda v: v) if CONFIGS[c]['SEPARATE_MULTIHEAD'] else (lambda v: None if v is None else v[0])
    bc, bb = head.generate_predicted_boxes(B, one(cls), one(box), one(d))
    if CONFIGS[c]['SEPARATE_MULTIHEAD']:
        assert isinstance(bc, list) and all(x is y for x, y in zip(bc, cls))
    check_decode(c, bb.cpu().numpy())
    if LAYOUT[c][1]:      # the restatement rounds where the kernel rounds
        ref = crs.decode(G[c + '_box_preds'].astype(np.float32), None, G[c + '_table'], sincos=1)
        assert ulps(bb.cpu().numpy()[..., 6], ref[..., 6]).max() <= 1


@gpu
def test_gpu_multi_classes_nms_with_nine_columns():
    """post_n: boxes (all 9 columns), labels, counts and order equal, scores within 2 ulp; nothing is read back."""
    rows, _, _ = layout('n')
    head = make_head('n')
    batch = {'batch_size': B, 'batch_cls_preds': [dev(G['post_n_cls_%d' % h]) for h in range(len(rows))],
             'batch_box_preds': dev(G['post_n_boxes']), 'cls_preds_normalized': False, 'gt_boxes': dev(G['post_n_gt_boxes']),
             'multihead_label_mapping': [h.head_label_indices.cuda() for h in head.rpn_heads]}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        padded = model_nms_utils.post_processing(batch, to_attr(POST), 5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    num = padded['num_pred'].cpu().numpy()
    assert np.array_equal(num, G['post_n_num_pred']) and padded['pred_labels'].dtype == torch.int64
    assert padded['pred_boxes'].shape == (B, G['post_n_pred_boxes'].shape[1], 9)
    assert np.array_equal(padded['pred_labels'].cpu().numpy(), G['post_n_pred_labels'])
    assert bits_equal(padded['pred_boxes'].cpu().numpy(), G['post_n_pred_boxes'])
    assert ulps(padded['pred_scores'].cpu().numpy(), G['post_n_pred_scores']).max() <= 2
    preds, recall = model_nms_utils.to_pred_and_recall_dicts(padded, POST['RECALL_THRESH_LIST'])
    assert recall == json.loads(str(G['post_n_recall']))
    assert [tuple(d['pred_boxes'].shape) for d in preds] == [(int(k), 9) for k in num]


@gpu
def test_gpu_no_host_read_and_graph_replay():
    """The head of configuration n: forward + get_loss + backward read nothing back (sync debug mode 'error'), are captured once
    and replayed; the replay's loss terms and the gradients of every prediction are the bits of the eager run."""
    torch.manual_seed(11)
    head = make_head('n').cuda().train()
    feats = torch.randn(B, 16, 9, 11, device='cuda')
    gt = dev(G['nx_gt_boxes'])
    params = [p for p in head.parameters()]

    def step():
        head({'spatial_features_2d': feats, 'gt_boxes': gt, 'batch_size': B})
        loss, tb = head.get_loss()
        preds = head.forward_ret_dict['cls_preds'] + head.forward_ret_dict['box_preds']
        grads = torch.autograd.grad(loss, preds + params)
        return torch.stack([tb[k] for k in tb]), grads[:len(preds)], grads[len(preds):]

    step()                                                     # uploads the anchor table, the one host-to-device copy
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        terms, g_preds, g_params = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    eager = [terms.clone()] + [g.clone() for g in g_preds]
    assert torch.isfinite(terms).all() and all(torch.isfinite(g).all() for g in g_params) and any(g.abs().max() > 0 for g in g_params)
    assert np.array_equal(head.forward_ret_dict['box_cls_labels'].cpu().numpy(), G['nx_box_cls_labels'])
    del terms, g_preds, g_params
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    head.forward_ret_dict.clear()                              # nothing of an earlier iteration may be alive at the capture
    gc.collect()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        terms_g, g_preds_g, g_params_g = step()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, [terms_g] + list(g_preds_g)):
        assert torch.equal(x, y), "the replay differs from the eager run"
    assert all(torch.isfinite(g).all() for g in g_params_g)


def scene_batch(name, counts, max_points, max_voxels, padded=False):
    from pdanet_amd.voxel_utils import VoxelGenerator, collate_voxels, collate_voxels_padded
    ds = dataset_of(name)
    rng = np.random.default_rng(5)
    pcr = np.array(ds['point_cloud_range'], np.float64)
    pts = np.concatenate([np.concatenate([rng.uniform(pcr[:3], pcr[3:], (n, 3)), rng.random((n, 2))], axis=1) for n in counts])
    offs = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64).cuda()
    gen = VoxelGenerator(ds['voxel_size'], ds['point_cloud_range'], 5, max_points, max_voxels)
    raw = gen.generate_batch((dev(pts.astype(np.float32)), offs, max(counts)))
    cx, cy = (pcr[0] + pcr[3]) / 2, (pcr[1] + pcr[4]) / 2
    gt = np.zeros((B, 3, 10), np.float32)
    gt[0, 0] = [cx, cy, -1.0, 4.63, 1.97, 1.74, 0.3, 0.5, np.nan, 1]              # car, vy unknown
    gt[0, 1] = [cx + 0.2, cy - 0.1, -0.6, 0.73, 0.67, 1.77, 1.2, np.nan, np.nan, 9]     # pedestrian, no velocity
    gt[1, 0] = [cx - 0.1, cy + 0.1, -0.6, 2.11, 0.77, 1.47, -0.4, -1.25, 0.75, 7]  # motorcycle
    batch = {'gt_boxes': dev(gt), 'batch_size': B}
    if padded:
        keys = ('voxels', 'voxel_coords', 'voxel_num_points', 'voxel_num_active', 'voxel_status')
        batch.update(zip(keys, collate_voxels_padded(*raw)))
    else:
        batch.update(zip(('voxels', 'voxel_coords', 'voxel_num_points'), collate_voxels(*raw)))
    return batch


def train_and_eval(name, batch):
    cfg = STATE[name]['config']
    torch.manual_seed(3)
    model = nuscenes_multihead.build(to_attr(cfg['MODEL']), 10, dataset_of(name)).cuda()
    model.train()
    ret, tb, disp = model(dict(batch))
    assert torch.isfinite(ret['loss']) and disp == {}
    assert set(tb) == {'loss_rpn', 'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss'}
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 and v.is_cuda for v in tb.values())
    assert int(model.dense_head.forward_ret_dict['num_pos'].sum()) > 0 and float(tb['rpn_loss_loc']) > 0
    ret['loss'].backward()
    for pname, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), pname
    heads = model.dense_head.rpn_heads
    assert all(h.conv_cls[-1].weight.grad.abs().max() > 0 for h in heads)
    for h in (0, 4, 5):      # the heads of car, motorcycle and pedestrian regress their positives
        assert any(p.grad.abs().max() > 0 for p in heads[h].conv_box.parameters()), h
    model.eval()
    with torch.no_grad():
        pred_dicts, recall = model(dict(batch))
    assert len(pred_dicts) == B and set(pred_dicts[0]) == {'pred_boxes', 'pred_scores', 'pred_labels'}
    assert all(d['pred_boxes'].shape == (len(d['pred_scores']), 9) and d['pred_labels'].dtype == torch.int64 for d in pred_dicts)
    assert all(((d['pred_labels'] >= 1) & (d['pred_labels'] <= 10)).all() for d in pred_dicts)
    assert set(recall) == {'gt', 'roi_0.3', 'rcnn_0.3', 'roi_0.5', 'rcnn_0.5', 'roi_0.7', 'rcnn_0.7'} and recall['gt'] == 3
    reference = {k: torch.zeros(shape) for k, shape in STATE[name]['state_dict']}
    fresh = nuscenes_multihead.build(to_attr(cfg['MODEL']), 10, dataset_of(name))
    fresh.load_state_dict(reference, strict=True)
    return model, float(ret['loss'].detach())


@gpu
def test_gpu_pointpillar_multihead_train_and_eval():
    """nuscenes_models/cbgs_pp_multihead.yaml's MODEL block on a 44 x 36 pillar grid: an 11 x 9 map, 1980 anchors a scene."""
    model, _ = train_and_eval('PointPillar', scene_batch('PointPillar', [1500, 900], 20, 1600))
    assert model.dense_head.anchor_table('cuda').shape == (10 * 2 * 11 * 9, 7)


@gpu
def test_gpu_second_net_multihead_train_and_eval():
    """nuscenes_models/cbgs_second_multihead.yaml's MODEL block (VoxelResBackBone8x) on the smallest grid of the 8x backbone,
    with the collated batch and with the padded one, which gives the same loss."""
    _, loss = train_and_eval('SECONDNet', scene_batch('SECONDNet', [1500, 900], 10, 2000))
    _, loss_padded = train_and_eval('SECONDNet', scene_batch('SECONDNet', [1500, 900], 10, 2000, padded=True))
    assert abs(loss - loss_padded) <= 1e-5 * abs(loss)
