"""AnchorHeadMulti, its class-major target assignment and ragged loss, the batched multi-class NMS and SECONDNet with the head of
kitti_models/second_multihead.yaml, against tests/golden/anchor_head_multi.npz: the reference's own AnchorHeadMulti,
AxisAlignedTargetAssigner and post_processing / multi_classes_nms on CPU tensors (tests/golden/make_anchor_head_multi_golden.py).

CPU part: the symbols, argument validation before any HIP call, the refusals of the contract (and that the old ones still
hold), the state-dict keys and anchors bit for bit, SECONDNet from the yaml's model block, and the float64 restatement
(tests/golden/anchor_head_multi_restatement.py) against the fixture.  GPU part: the kernels against the same fixture.

Tolerances are those of tests/test_anchor_head.py, whose rule for the targets and LOSS_TOL are imported: labels, weights and
counts equal; target columns 0-2 and 6 bit-identical, the log columns within one float32 ulp; losses within 2e-5, gradients
within 2e-5 of the largest reference gradient.  Multi-class NMS: boxes, labels, counts and the order equal; the scores are
torch.sigmoid on another device, compared within 2 float32 ulp (the maker keeps the scores of a column 1e-5 apart and 1e-4
away from the threshold, so neither the order nor the mask can depend on that)."""
import ctypes
import gc
import json
import os
import sys

import numpy as np
import pytest
import torch

from pdanet_amd import _lib, anchor_head as ah, anchor_head_multi as ahm, build, model_nms_utils
from pdanet_amd.config import to_attr
from pdanet_amd.second_net import SECONDNet

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import anchor_head_multi_restatement as mrs  # noqa: E402
import anchor_head_restatement as rs  # noqa: E402
from test_anchor_head import LOSS_TOL, bits_equal, ulps  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "anchor_head_multi.npz")
G = np.load(FIXTURE)
SETUP = json.loads(str(G['configs']))
CONFIGS, POST, CLASS_NAMES = SETUP['heads'], SETUP['post'], SETUP['class_names']
B = 2
BATCHES = [(c, t) for c in 'abc' for t in 'xyz']
KEYS = ['rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir', 'rpn_loss']


def make_head(c, input_channels=16, cls=ahm.AnchorHeadMulti, **over):
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
    return cls(model_cfg=to_attr(head_cfg), input_channels=input_channels, num_class=3, class_names=CLASS_NAMES, grid_size=grid,
               point_cloud_range=pcr, predict_boxes_when_training=False)


def class_arrays(c):
    gen = CONFIGS[c]['ANCHOR_GENERATOR_CONFIG']
    return ([CLASS_NAMES.index(g['class_name']) + 1 for g in gen], [g['matched_threshold'] for g in gen],
            [g['unmatched_threshold'] for g in gen], [int(v) for v in G[c + '_class_rows']])


def layout(c):
    """Per prediction tensor of the loss: its rows, logit columns and column base (one tensor when not separate)."""
    class_rows = [int(v) for v in G[c + '_class_rows']]
    if not CONFIGS[c]['SEPARATE_MULTIHEAD']:
        return [sum(class_rows)], [3], [0]
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
    full = [G['%s_%s_preds' % (c, k)].astype(np.float32) if '%s_%s_preds' % (c, k) in G else None for k in ('cls', 'box', 'dir')]
    out = []
    for i, x in enumerate(full):
        if x is None:
            out.append(None)
            continue
        parts, at = [], 0
        for h, n in enumerate(rows):
            part = x[:, at:at + n]
            if i == 0 and len(rows) > 1:
                part = part[..., bases[h]:bases[h] + cols[h]]
            parts.append(np.ascontiguousarray(part))
            at += n
        out.append(parts)
    return out


def check_targets(c, t, labels, targets, weights, num_pos):
    """The rule of tests/test_anchor_head.py check_targets, on this fixture."""
    p = c + t + '_'
    ref_l, ref_t, ref_w = G[p + 'box_cls_labels'], G[p + 'box_reg_targets'], G[p + 'reg_weights']
    assert labels.dtype == np.int32 and labels.shape == ref_l.shape
    assert np.array_equal(labels, ref_l), "labels"
    assert bits_equal(weights, ref_w), "reg_weights"
    assert np.array_equal(num_pos, (ref_l > 0).sum(axis=1)), "num_pos"
    assert bits_equal(targets[..., [0, 1, 2, 6]], ref_t[..., [0, 1, 2, 6]]), "centre and heading targets"
    d = ulps(targets[..., 3:6], ref_t[..., 3:6])
    print("targets", c, t, "log columns off by one ulp at", int((d != 0).sum()), "of", int((ref_l > 0).sum()) * 3)
    assert d.max() <= 1, "log targets"


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


NAMES = ["pda_anchor_multi_assign_targets", "pda_anchor_multi_loss_blocks", "pda_anchor_multi_loss", "pda_multi_nms_compact"]


def test_symbols_exported(lib):
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.pda_abi_version() == 20


def test_fixture_is_small_and_covers_the_cases():
    assert os.path.getsize(FIXTURE) < 1 << 20
    assert G['a_table'].shape == (594, 7) and G['b_table'].shape == (891, 7) and G['c_table'].shape == (891, 7)
    assert list(G['a_class_rows']) == [198, 198, 198] and list(G['b_class_rows']) == [198, 396, 297]
    for c in 'abc':
        assert all(int(r) % 64 for r in G[c + '_class_rows']) and len(G[c + '_table']) % 64 and len(G[c + '_table']) % 256
        gt = G[c + 'x_gt_boxes'][0]
        assert bits_equal(gt[0], gt[1])                                        # two identical boxes
        zero = ~gt.any(axis=1)
        assert zero[6] and not zero[7] and zero[-3:].all()                      # an interior zero row, trailing zero rows
        lab, mx, umx, class_rows = class_arrays(c)
        cls_of = np.repeat(np.arange(len(lab)), class_rows)
        iou = np.concatenate([G['%sx_iou_%d' % (c, i)] for i in range(len(lab))], axis=0)
        labels = G[c + 'x_box_cls_labels'][0]
        assert iou[:, 4].max() == 0                                             # a box that overlaps no anchor
        sq = iou[:, 2] * (np.array(lab)[cls_of] == gt[2, 7])
        assert (sq == sq.max()).sum() >= 2 and (labels[sq == sq.max()] > 0).all()      # a tie for the column maximum
        sm = iou[:, 3] * (np.array(lab)[cls_of] == gt[3, 7])
        un = np.array(umx)[cls_of][sm == sm.max()]
        assert (sm.max() < un).all() and (labels[sm == sm.max()] > 0).all()     # a forced positive below unmatched
        assert (labels < 0).any() and (G[c + 'z_box_cls_labels'] == 0).all()    # a batch without gts
        assert (G[c + 'y_box_cls_labels'][0] == 0).all()                        # a scene without gts
        only = G[c + 'x_box_cls_labels'][1]                                     # gts of one class: the other heads background
        assert (only[:class_rows[0]] > 0).any() and (only[class_rows[0]:] == 0).all()
    assert layout('a') == ([198] * 3, [1, 1, 1], [0, 1, 2]) and layout('b') == ([198, 693], [1, 2], [0, 1])
    assert layout('c') == ([891], [3], [0]) and 'c_dir_preds' not in G and 'b_dir_preds' in G
    pre, post = POST['NMS_CONFIG']['NMS_PRE_MAXSIZE'], POST['NMS_CONFIG']['NMS_POST_MAXSIZE']
    for c in 'ab':
        rows, cols, _ = layout(c)
        thr = np.log(POST['SCORE_THRESH'] / (1 - POST['SCORE_THRESH']))
        above = [(G['post_%s_cls_%d' % (c, h)] >= thr).sum(axis=1) for h in range(len(rows))]
        assert min(rows) > pre and max(int(a.max()) for a in above) > pre       # NMS_PRE_MAXSIZE truncates
        assert min(int(a.min()) for a in above) == 0                            # a column with nothing above the threshold
        counts = [np.bincount(G['post_%s_pred_labels' % c][s, :G['post_%s_num_pred' % c][s]], minlength=4) for s in range(B)]
        assert max(int(v.max()) for v in counts) == post and counts[1][3] == 0 and counts[0][3] > 0


def test_argument_validation_without_gpu(lib):
    i64, d = ctypes.c_int64, ctypes.c_double
    lab = (ctypes.c_int32 * 2)(1, 2)
    thr = (ctypes.c_float * 2)(0.6, 0.5)
    rows = (ctypes.c_int32 * 2)(5, 3)
    assign = lambda cols, b, m, n, n_cls, label=lab, count=rows: lib.pda_anchor_multi_assign_targets(
        None, cols, b, m, None, n, n_cls, label, thr, thr, count, None, None, None, None, None, None)
    assert assign(10, 1, 4, 8, 2) == 1 and b"gt_cols" in lib.pda_last_error()
    assert assign(8, -1, 4, 8, 2) == 1
    assert assign(8, 1, 4, 8, 0) == 1 and b"n_cls" in lib.pda_last_error()
    assert assign(8, 0, 4, 8, 2) == 0                                           # the empty problem
    assert assign(8, 1, 4, 8, 2, label=(ctypes.c_int32 * 2)(1, 1)) == 1 and b"share label" in lib.pda_last_error()
    assert assign(8, 1, 4, 9, 2) == 1 and b"rows" in lib.pda_last_error()       # the classes own 8 rows of 9
    assert assign(8, 1, 4, 7, 2) == 1 and b"rows" in lib.pda_last_error()
    assert assign(8, 1, 4, 8, 2, count=(ctypes.c_int32 * 2)(8, 0)) == 1 and b"class_count" in lib.pda_last_error()
    assert assign(8, 1, 4, 8, 2) == 1 and b"null" in lib.pda_last_error()
    assert lib.pda_anchor_multi_loss_blocks(i64(0)) == 0 and lib.pda_anchor_multi_loss_blocks(i64(1)) == 1
    assert lib.pda_anchor_multi_loss_blocks(i64(1025)) == 2 and lib.pda_anchor_multi_loss_blocks(i64(1 << 30)) == 2048
    w = (ctypes.c_float * 7)(*[1.0] * 7)
    ptrs = (ctypes.c_void_p * 2)(None, None)
    cols, base = (ctypes.c_int32 * 2)(1, 2), (ctypes.c_int32 * 2)(0, 1)
    loss = lambda b, n, heads, nc=3, hrows=rows, hcols=cols: lib.pda_anchor_multi_loss(
        ptrs, ptrs, ptrs, heads, hrows, hcols, base, None, None, None, None, b, n, nc, 2, w, d(1), d(2), d(0.2), d(0.78), d(1), d(1),
        ptrs, ptrs, ptrs, None, None, None)
    assert loss(0, 8, 2) == 1 and loss(1, 8, 0) == 1 and b"n_heads" in lib.pda_last_error()
    assert loss(1, 8, 33) == 1 and b"n_heads" in lib.pda_last_error()
    assert loss(1, 8, 2, hcols=(ctypes.c_int32 * 2)(4, 2)) == 1 and b"columns" in lib.pda_last_error()      # 0..4 of 3 classes
    assert loss(1, 8, 2) == 1 and b"null pointer of head 0" in lib.pda_last_error()
    compact = lambda b, c, k, post: lib.pda_multi_nms_compact(None, None, None, None, None, b, c, k, post, None, None, None, None, None)
    assert compact(-1, 3, 8, 4) == 1 and compact(1, 0, 8, 4) == 1 and b"problems" in lib.pda_last_error()
    assert compact(1, 257, 8, 4) == 1 and compact(0, 3, 8, 4) == 0 and compact(1, 3, 8, 4) == 1 and b"null" in lib.pda_last_error()


def test_out_of_contract_is_refused():
    for over in ({'TARGET_ASSIGNER_CONFIG__POS_FRACTION': 0.5}, {'TARGET_ASSIGNER_CONFIG__NORM_BY_NUM_EXAMPLES': True},
                 {'TARGET_ASSIGNER_CONFIG__MATCH_HEIGHT': True}, {'TARGET_ASSIGNER_CONFIG__NAME': 'ATSS'},
                 {'USE_MULTIHEAD': False}, {'TARGET_ASSIGNER_CONFIG__BOX_CODER_CONFIG': {'encode_angle_by_sincos': True}},
                 {'TARGET_ASSIGNER_CONFIG__BOX_CODER_CONFIG': {'code_size': 9}}):
        with pytest.raises(NotImplementedError):
            make_head('a', **over)
    gen = json.loads(json.dumps(CONFIGS['a']['ANCHOR_GENERATOR_CONFIG']))
    gen[1]['anchor_bottom_heights'] = [-1.6, -0.6]
    with pytest.raises(NotImplementedError, match="bottom height"):
        make_head('a', ANCHOR_GENERATOR_CONFIG=gen)
    with pytest.raises(ValueError, match="order"):
        make_head('b', RPN_HEAD_CFGS=[{'HEAD_CLS_NAME': ['Pedestrian', 'Cyclist']}, {'HEAD_CLS_NAME': ['Car']}])
    with pytest.raises(AssertionError, match="Code size"):
        make_head('c', SEPARATE_REG_CONFIG={'NUM_MIDDLE_CONV': 1, 'NUM_MIDDLE_FILTER': 8, 'REG_LIST': ['reg:2', 'size:3']})
    head = make_head('a')
    with pytest.raises(NotImplementedError, match="7 \\+ 1"):
        head.target_assigner.assign_targets(head.anchors, torch.zeros(1, 4, 10))
    # the old refusals hold: AnchorHeadSingle and its assigner with USE_MULTIHEAD, a single tensor with MULTI_CLASSES_NMS
    with pytest.raises(NotImplementedError, match="USE_MULTIHEAD"):
        make_head('a', cls=ah.AnchorHeadSingle, RPN_HEAD_CFGS=None)
    coder = head.box_coder
    with pytest.raises(NotImplementedError, match="USE_MULTIHEAD"):
        ah.AxisAlignedTargetAssigner(to_attr(CONFIGS['a']), CLASS_NAMES, coder)
    with pytest.raises(NotImplementedError, match="USE_MULTIHEAD"):
        ahm.ClassMajorTargetAssigner(to_attr(dict(CONFIGS['a'], USE_MULTIHEAD=False)), CLASS_NAMES, coder)
    batch = {'batch_size': 1, 'batch_cls_preds': torch.zeros(1, 4, 3), 'batch_box_preds': torch.zeros(1, 4, 7), 'cls_preds_normalized': False}
    with pytest.raises(NotImplementedError, match="MULTI_CLASSES_NMS"):
        model_nms_utils.post_processing(batch, POST, 3)


def test_no_cpu_path():
    head = make_head('a')
    with pytest.raises(RuntimeError, match="no CPU path"):
        head.assign_targets(torch.zeros(1, 4, 8))
    cls, box, d = ([torch.from_numpy(v) for v in parts] for parts in preds_of('a'))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ahm.anchor_multi_loss(cls, box, d, [1, 1, 1], [0, 1, 2], torch.from_numpy(G['ax_box_cls_labels']),
                              torch.from_numpy(G['ax_box_reg_targets']), torch.zeros(2, dtype=torch.int32),
                              torch.from_numpy(G['a_table']), 3, [1.0] * 7, 1.0, 2.0, 0.2, 0.78539)
    batch = {'batch_size': 2, 'batch_cls_preds': cls, 'batch_box_preds': torch.zeros(2, 594, 7), 'cls_preds_normalized': False,
             'multihead_label_mapping': [torch.tensor([i + 1]) for i in range(3)]}
    with pytest.raises(RuntimeError, match="no CPU path"):
        model_nms_utils.post_processing(batch, POST, 3)


def test_state_dict_keys_and_anchors_are_the_references():
    for c in 'abc':
        head = make_head(c)
        sd = head.state_dict()
        assert list(sd.keys()) == [str(k) for k in G['keys_' + c]]
        assert [list(v.shape) for v in sd.values()] == json.loads(str(G['shapes_' + c]))
        head.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
        for i, a in enumerate(head.anchors):
            assert bits_equal(a.numpy(), G['%s_anchors_%d' % (c, i)]), "anchors of class %d" % i
        table, class_rows = ahm.class_major_table(head.anchors)
        assert bits_equal(table.numpy(), G[c + '_table']) and class_rows == [int(v) for v in G[c + '_class_rows']]
        assert sum(head.head_rows) == len(table) and head.head_rows == (layout(c)[0] if c != 'c' else [198, 693])
        rs_table, rs_rows = mrs.class_major_table([a.numpy() for a in head.anchors])
        assert bits_equal(rs_table, G[c + '_table']) and rs_rows == class_rows
    b = make_head('b')
    assert [h.num_class for h in b.rpn_heads] == [1, 2] and [h.num_class for h in make_head('c').rpn_heads] == [3, 3]
    assert [h.head_label_indices.tolist() for h in b.rpn_heads] == [[1], [2, 3]]
    assert abs(float(b.rpn_heads[1].conv_cls.bias[0].detach()) + np.log(99.0)) < 1e-6 and make_head('a').shared_conv is not None
    assert any(k.startswith('rpn_heads.1.blocks.0.') for k in G['keys_c']) and any('conv_box.conv_reg.' in k for k in G['keys_c'])


def test_second_net_builds_from_the_yaml():
    y = json.loads(str(G['yaml']))
    assert y['MODEL']['DENSE_HEAD']['NAME'] == 'AnchorHeadMulti' and y['MODEL']['POST_PROCESSING']['NMS_CONFIG']['MULTI_CLASSES_NMS']
    model = SECONDNet(to_attr(y['MODEL']), 3, dict(y['dataset'], class_names=CLASS_NAMES, num_point_features=4))
    assert [n for n, _ in model.named_children()] == ['vfe', 'backbone_3d', 'map_to_bev_module', 'backbone_2d', 'dense_head']
    assert isinstance(model.dense_head, ahm.AnchorHeadMulti) and model.dense_head.head_rows == [2 * 200 * 176] * 3
    assert [[k, list(v.shape)] for k, v in model.dense_head.state_dict().items()] == y['head_state_dict']


@pytest.mark.parametrize("c", "abc")
def test_restatement_iou(c):
    lab, mx, umx, class_rows = class_arrays(c)
    first = np.concatenate([[0], np.cumsum(class_rows)])
    for i in range(len(lab)):
        got = rs.nearest_bev_iou(G[c + '_table'][first[i]:first[i + 1]], G[c + 'x_gt_boxes'][0][:, :7])
        assert bits_equal(got, G['%sx_iou_%d' % (c, i)]), "IoU of class %d" % i


@pytest.mark.parametrize("c,t", BATCHES)
def test_restatement_targets(c, t):
    check_targets(c, t, *mrs.assign_targets(G[c + t + '_gt_boxes'], G[c + '_table'], *class_arrays(c)))


def loss_weights(c):
    cfg = CONFIGS[c]
    w = cfg['LOSS_CONFIG']['LOSS_WEIGHTS']
    return dict(num_class=3, code_weights=w['code_weights'], cls_weight=w['cls_weight'], loc_weight=w['loc_weight'],
                dir_weight=w['dir_weight'], dir_offset=cfg.get('DIR_OFFSET', 0.0))


@pytest.mark.parametrize("c,t", BATCHES)
def test_restatement_losses(c, t):
    p = c + t + '_'
    cls, box, d = preds_of(c)
    _, cols, bases = layout(c)
    got = mrs.losses(cls, box, d, cols, bases, G[p + 'box_cls_labels'], G[p + 'box_reg_targets'], G[c + '_table'], **loss_weights(c))
    assert np.abs(got - G[p + 'losses']).max() <= LOSS_TOL


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
    assert bits_equal(gt.cpu().numpy(), before.cpu().numpy()), "gt_boxes was written"


@gpu
def test_gpu_targets_do_not_depend_on_order():
    for c in 'ab':
        head = make_head(c).cuda()
        gt = dev(G[c + 'x_gt_boxes'])
        _, first = run_targets(head, gt)
        _, again = run_targets(head, gt)
        for x, y in zip(first, again):
            assert bits_equal(x, y), "two runs differ"


@gpu
def test_gpu_targets_more_gts_than_a_tile():
    """m = 70 boxes of one class on configuration b: more than one 64-row tile; against the restatement."""
    rng = np.random.default_rng(7)
    pcr = SETUP['point_cloud_range']
    m = 70
    gt = np.zeros((1, m, 8), np.float32)
    gt[0, :, 0] = rng.uniform(pcr[0], pcr[3], m)
    gt[0, :, 1] = rng.uniform(pcr[1], pcr[4], m)
    gt[0, :, 2] = -1.0
    gt[0, :, 3:6] = np.array([0.8, 0.6, 1.73]) * rng.uniform(0.8, 1.2, (m, 3))
    gt[0, :, 6] = rng.uniform(-3, 3, m)
    gt[0, :, 7] = 2
    gt[0, 20] = 0                                                              # an interior zero row
    head = make_head('b').cuda()
    _, (labels, targets, weights, num_pos) = run_targets(head, dev(gt))
    ref = mrs.assign_targets(gt, G['b_table'], *class_arrays('b'))
    assert np.array_equal(labels, ref[0]) and np.array_equal(num_pos, ref[3]) and bits_equal(weights, ref[2])
    assert (labels > 0).sum() > 64 and (labels[0, :198] == 0).all() and (labels[0, 594:] == 0).all()
    assert bits_equal(targets[..., [0, 1, 2, 6]], ref[1][..., [0, 1, 2, 6]]) and ulps(targets[..., 3:6], ref[1][..., 3:6]).max() <= 1


def single_head_and_permutation():
    """AnchorHeadSingle on configuration a's anchors (all classes share stride and rotations) and perm with
    class-major row i == location-major row perm[i]."""
    single = make_head('a', cls=ah.AnchorHeadSingle, USE_MULTIHEAD=None, SEPARATE_MULTIHEAD=None, RPN_HEAD_CFGS=None,
                       SHARED_CONV_NUM_FILTER=None)
    ny, nx = single.anchors[0].shape[1:3]
    c, a, y, x = np.meshgrid(np.arange(3), np.arange(2), np.arange(ny), np.arange(nx), indexing='ij')
    perm = (((y * nx + x) * 3 + c) * 2 + a).reshape(-1)
    assert bits_equal(ah.anchor_table(single.anchors)[0].numpy()[perm], G['a_table'])
    return single, perm


@gpu
def test_gpu_targets_equal_the_single_heads_permuted():
    single, perm = single_head_and_permutation()
    multi = make_head('a').cuda()
    gt = dev(G['ax_gt_boxes'])
    _, got = run_targets(multi, gt)
    _, ref = run_targets(single.cuda(), gt)
    for x, y in zip(got[:3], ref[:3]):
        assert bits_equal(x, y[:, perm])
    assert np.array_equal(got[3], ref[3])


def head_loss(head, c, t):
    leaves = [None if parts is None else [dev(v).requires_grad_(True) for v in parts] for parts in preds_of(c)]
    one = (lambda v: v) if CONFIGS[c]['SEPARATE_MULTIHEAD'] else (lambda v: v[0])
    head.forward_ret_dict = dict({'cls_preds': one(leaves[0]), 'box_preds': one(leaves[1])},
                                 **head.assign_targets(dev(G[c + t + '_gt_boxes'])))
    if leaves[2] is not None:
        head.forward_ret_dict['dir_cls_preds'] = one(leaves[2])
    loss, tb = head.get_loss()
    return loss, tb, leaves


def check_losses(c, t, tb, leaves):
    p = c + t + '_'
    ref = G[p + 'losses']
    has_dir = leaves[2] is not None
    assert list(tb) == (KEYS if has_dir else [k for k in KEYS if k != 'rpn_loss_dir'])
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 and v.is_cuda for v in tb.values())
    d_loss = [abs(float(tb[k]) - float(ref[i])) for i, k in enumerate(KEYS) if k in tb]
    refs, grads = [], []
    for name, parts in zip(('cls', 'box', 'dir'), leaves):
        for h, v in enumerate(parts or []):
            refs.append(G['%sg_%s_%d' % (p, name, h)])
            grads.append(v.grad.cpu().numpy())
            assert grads[-1].shape == refs[-1].shape
    scale = max(float(np.abs(v).max()) for v in refs)
    d_g = max(float(np.abs(g.astype(np.float64) - r).max()) for g, r in zip(grads, refs))
    print("loss", c, t, "terms", ["%.3g" % v for v in d_loss], "grad %.3g of %.3g" % (d_g, scale))
    assert max(d_loss) <= LOSS_TOL
    assert d_g <= LOSS_TOL * scale


@gpu
@pytest.mark.parametrize("c,t", BATCHES)
def test_gpu_losses(c, t):
    head = make_head(c).cuda()
    before = dev(G[c + t + '_box_cls_labels'])
    loss, tb, leaves = head_loss(head, c, t)
    loss.backward()
    check_losses(c, t, tb, leaves)
    assert float(loss.detach()) == float(tb['rpn_loss'])
    assert torch.equal(head.forward_ret_dict['box_cls_labels'], before), "the labels were rewritten"


def loss_case(n):
    """One scene of n anchors: a head of one logit column over the first third of the rows and one of two columns (column
    base 1) over the rest (one head when n == 1), two direction bins, logits around -4, about 5 % ignored anchors, up to five
    positives (the first and the last anchor among them), one of them with a NaN regression target."""
    rng = np.random.default_rng(n)
    rows = [n] if n == 1 else [n // 3, n - n // 3]
    cols, bases = ([1], [0]) if n == 1 else ([1, 2], [0, 1])
    table = np.zeros((n, 7), np.float32)
    table[:, :2] = rng.uniform(-40, 40, (n, 2))
    table[:, 3:6] = (3.9, 1.6, 1.56)
    table[:, 6] = rng.choice(np.array([0.0, 1.57], np.float32), n)
    cls = [rng.normal(-4.0, 1.0, (1, r, k)).astype(np.float32) for r, k in zip(rows, cols)]
    box = [rng.normal(0.0, 0.3, (1, r, 7)).astype(np.float32) for r in rows]
    dirs = [rng.normal(0.0, 1.0, (1, r, 2)).astype(np.float32) for r in rows]
    labels = np.where(rng.random((1, n)) < 0.05, -1, 0).astype(np.int32)
    pos = np.unique(np.linspace(0, n - 1, min(n, 5)).astype(np.int64))
    labels[0, pos] = np.where(pos < rows[0], 1, 2 + (pos % 2)).astype(np.int32)      # a head's positives carry its labels
    targets = np.zeros((1, n, 7), np.float32)
    targets[0, pos] = rng.normal(0.0, 0.3, (len(pos), 7))
    targets[0, pos[0], 2] = np.nan
    return cls, box, dirs, cols, bases, labels, targets, np.array([len(pos)], np.int32), table


LOSS_CASE_WEIGHTS = dict(num_class=3, code_weights=[1.0] * 7, cls_weight=1.0, loc_weight=2.0, dir_weight=0.2, dir_offset=0.78539)


@gpu
@pytest.mark.parametrize("n,blocks,more", [(1, 1, {}), (1025, 2, {'pos_cls_weight': 2.0, 'neg_cls_weight': 0.5}), (2097153, 2048, {})])
def test_gpu_multi_loss_at_the_block_boundaries(n, blocks, more):
    """The sizes at which the shared partial sums (csrc/loss_sums.h) can go wrong, from pda_anchor_multi_loss_blocks: one
    anchor; one full workgroup of 1024 and one anchor; one anchor past the 2048-workgroup cap, where the grid-stride loop
    wraps.  Against the float64 restatement, within test_gpu_losses' bound.  The middle case also weighs positives and negatives
    differently (LOSS_WEIGHTS pos_cls_weight / neg_cls_weight, which no fixture configuration sets)."""
    assert _lib.load().pda_anchor_multi_loss_blocks(n) == blocks
    cls, box, dirs, cols, bases, labels, targets, num_pos, table = loss_case(n)
    ref = mrs.losses(cls, box, dirs, cols, bases, labels, targets, table, **LOSS_CASE_WEIGHTS, **more)
    leaves = [[dev(v).requires_grad_(True) for v in parts] for parts in (cls, box, dirs)]
    loss, out = ahm.anchor_multi_loss(*leaves, cols, bases, dev(labels), dev(targets), dev(num_pos), dev(table), **LOSS_CASE_WEIGHTS,
                                      **more)
    loss.backward()
    d_loss = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    print("multi n", n, "losses", ref, "diff", ["%.3g" % v for v in d_loss])
    assert d_loss.max() <= LOSS_TOL
    assert float(loss.detach()) == float(out[3])
    g_box = np.concatenate([v.grad.cpu().numpy() for v in leaves[1]], axis=1)
    assert all(bool(torch.isfinite(v.grad).all()) for parts in leaves for v in parts) and g_box[0, 0, 2] == 0      # the NaN target
    assert g_box[0, 0, [0, 1, 3, 4, 5, 6]].all() and not g_box[labels <= 0].any() and (n == 1 or g_box[0, -1].all())


def check_decode(c, boxes):
    """The rule of tests/test_anchor_head.py check_decode, on this fixture."""
    ref = G[c + '_batch_box_preds']
    assert boxes.shape == ref.shape
    assert bits_equal(boxes[..., :3], ref[..., :3]), "centres"
    assert ulps(boxes[..., 3:6], ref[..., 3:6]).max() <= 2, "sizes"
    if c + '_dir_preds' in G:
        assert ulps(boxes[..., 6], ref[..., 6]).max() <= 2, "heading behind the direction classifier"
    else:
        assert bits_equal(boxes[..., 6], ref[..., 6]), "heading"


@gpu
@pytest.mark.parametrize("c", "abc")
def test_gpu_decode(c):
    head = make_head(c).cuda().eval()
    cls, box, d = ([dev(v) for v in parts] if parts is not None else None for parts in preds_of(c))
    one = (lambda v: v) if CONFIGS[c]['SEPARATE_MULTIHEAD'] else (lambda v: None if v is None else v[0])
    bc, bb = head.generate_predicted_boxes(B, one(cls), one(box), one(d))
    if CONFIGS[c]['SEPARATE_MULTIHEAD']:
        assert isinstance(bc, list) and all(x is y for x, y in zip(bc, cls))
    else:
        assert bits_equal(bc.cpu().numpy(), G[c + '_cls_preds'].astype(np.float32))
    check_decode(c, bb.cpu().numpy())


@gpu
def test_gpu_decode_equals_the_single_heads():
    single, perm = single_head_and_permutation()
    single = single.cuda().eval()
    multi = make_head('a').cuda().eval()
    cls, box, d = ([dev(v) for v in parts] for parts in preds_of('a'))
    _, got = multi.generate_predicted_boxes(B, cls, box, d)
    inv = np.argsort(perm)                                       # location-major row j == class-major row inv[j]
    ny, nx = single.anchors[0].shape[1:3]
    as_map = lambda parts: torch.cat(parts, dim=1)[:, inv].reshape(B, ny, nx, -1).contiguous()
    _, ref = single.generate_predicted_boxes(B, torch.zeros(B, ny, nx, 18, device='cuda'), as_map(box), as_map(d))
    assert bits_equal(got.cpu().numpy(), ref.cpu().numpy()[:, perm])


def post_batch(c):
    rows, _, _ = layout(c)
    head = make_head(c)
    return {'batch_size': B, 'batch_cls_preds': [dev(G['post_%s_cls_%d' % (c, h)]) for h in range(len(rows))],
            'batch_box_preds': dev(G['post_%s_boxes' % c]), 'cls_preds_normalized': False, 'gt_boxes': dev(G['post_%s_gt_boxes' % c]),
            'multihead_label_mapping': [h.head_label_indices.cuda() for h in head.rpn_heads]}


@gpu
@pytest.mark.parametrize("c", "ab")
def test_gpu_multi_classes_nms(c):
    """Per scene, in order: boxes, labels and counts equal, scores within 2 ulp (a sigmoid on another device).  The fixture
    holds a column with nothing above the threshold, columns with more than NMS_POST_MAXSIZE survivors and heads with more
    rows (and more rows above the threshold) than NMS_PRE_MAXSIZE = 96."""
    batch = post_batch(c)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        padded = model_nms_utils.post_processing(batch, to_attr(POST), 3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    p = 'post_%s_' % c
    num = padded['num_pred'].cpu().numpy()
    assert np.array_equal(num, G[p + 'num_pred']) and padded['pred_labels'].dtype == torch.int64
    K = G[p + 'pred_boxes'].shape[1]
    assert padded['pred_boxes'].shape == (B, K, 7)
    assert np.array_equal(padded['pred_labels'].cpu().numpy(), G[p + 'pred_labels'])
    assert bits_equal(padded['pred_boxes'].cpu().numpy(), G[p + 'pred_boxes'])
    assert ulps(padded['pred_scores'].cpu().numpy(), G[p + 'pred_scores']).max() <= 2
    preds, recall = model_nms_utils.to_pred_and_recall_dicts(padded, POST['RECALL_THRESH_LIST'])
    assert recall == json.loads(str(G[p + 'recall']))
    assert [len(d['pred_scores']) for d in preds] == list(num)


def selection_head(c):
    """A head whose 1x1 convolutions copy channels of the input, so that a forward on the fixture's predictions laid out as a
    (B, C, H, W) map reproduces them exactly (1 * x plus zeros).  Without the shared convolution."""
    head = make_head(c, SHARED_CONV_NUM_FILTER=None)
    ny, nx = head.anchors[0].shape[1:3]
    parts = preds_of(c)
    maps, plan = [], []
    for h, rpn in enumerate(head.rpn_heads):
        A = rpn.num_anchors_per_location
        for conv, p in ((rpn.conv_cls, parts[0]), (rpn.conv_box, parts[1]), (rpn.conv_dir_cls, parts[2])):
            m = p[h].reshape(B, A, ny, nx, -1).transpose(0, 1, 4, 2, 3).reshape(B, -1, ny, nx)
            maps.append(m)
            plan.append((h, conv is rpn.conv_cls, conv is rpn.conv_box, m.shape[1]))
    head = make_head(c, input_channels=sum(m.shape[1] for m in maps), SHARED_CONV_NUM_FILTER=None).cuda().train()
    convs, off = [], 0
    with torch.no_grad():
        for h, is_cls, is_box, n in plan:
            rpn = head.rpn_heads[h]
            conv = rpn.conv_cls if is_cls else (rpn.conv_box if is_box else rpn.conv_dir_cls)
            conv.weight.zero_()
            conv.bias.zero_()
            conv.weight[torch.arange(n), off + torch.arange(n), 0, 0] = 1.0
            off += n
            convs.append(conv)
    return head, dev(np.concatenate(maps, axis=1)), convs


@gpu
def test_gpu_no_host_read_and_graph_replay():
    """forward + get_loss + backward read nothing back (sync debug mode 'error'), are captured once and replayed on a second
    batch: the replay gives that batch's fixture losses."""
    head, feats, convs = selection_head('b')
    params = [p for conv in convs for p in (conv.weight, conv.bias)]
    gt = dev(G['bx_gt_boxes'])

    def step():
        head({'spatial_features_2d': feats, 'gt_boxes': gt, 'batch_size': B})
        loss, tb = head.get_loss()
        return tb, torch.autograd.grad(loss, params)

    step()                                                     # uploads the anchor table, the one host-to-device copy
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tb, grads = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.abs(np.array([float(tb[k]) for k in KEYS]) - G['bx_losses']).max() <= LOSS_TOL
    assert all(g.abs().max() > 0 for g in grads)
    del tb, grads
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
        tb_g, grads_g = step()
    gt.copy_(dev(G['by_gt_boxes']))                            # the second batch, into the captured input
    graph.replay()
    torch.cuda.synchronize()
    assert np.abs(np.array([float(tb_g[k]) for k in KEYS]) - G['by_losses']).max() <= LOSS_TOL
    assert all(torch.isfinite(g).all() for g in grads_g)
    assert np.array_equal(head.forward_ret_dict['box_cls_labels'].cpu().numpy(), G['by_box_cls_labels'])


@gpu
def test_gpu_second_net_multihead_train_and_eval():
    from pdanet_amd.voxel_utils import VoxelGenerator, collate_voxels
    with open(os.path.join(HERE, "golden", "second_state_dict.json")) as f:
        small = json.load(f)['config']
    y = json.loads(str(G['yaml']))['MODEL']
    ds = small['dataset']
    stride = small['MODEL']['DENSE_HEAD']['ANCHOR_GENERATOR_CONFIG'][0]['feature_map_stride']
    head_cfg = json.loads(json.dumps(y['DENSE_HEAD']))
    for g in head_cfg['ANCHOR_GENERATOR_CONFIG']:
        g['feature_map_stride'] = stride
    cfg = dict(small['MODEL'], DENSE_HEAD=head_cfg, POST_PROCESSING=y['POST_PROCESSING'])
    torch.manual_seed(3)
    model = SECONDNet(to_attr(cfg), 3, ds).cuda()
    rng = np.random.default_rng(5)
    pcr = np.array(ds['point_cloud_range'], np.float64)
    counts = [1500, 900]                                       # a ragged scene pair
    pts = np.concatenate([np.concatenate([rng.uniform(pcr[:3], pcr[3:], (n, 3)), rng.random((n, 1))], axis=1) for n in counts])
    offs = torch.tensor([0, counts[0], sum(counts)], dtype=torch.int64).cuda()
    gen = VoxelGenerator(ds['voxel_size'], ds['point_cloud_range'], 4, 5, 2000)
    voxels, coords, num_points = collate_voxels(*gen.generate_batch((dev(pts.astype(np.float32)), offs, max(counts))))
    gt = np.zeros((B, 3, 8), np.float32)
    gt[0, 0] = [0.4, 0.0, -1.0, 3.9, 1.6, 1.56, 0.3, 1]
    gt[0, 1] = [0.3, 0.1, -0.6, 0.8, 0.6, 1.73, 1.2, 2]
    gt[1, 0] = [0.5, -0.1, -0.6, 1.76, 0.6, 1.73, -0.4, 3]
    batch = {'voxels': voxels, 'voxel_coords': coords, 'voxel_num_points': num_points, 'gt_boxes': dev(gt), 'batch_size': B}
    model.train()
    ret, tb, disp = model(dict(batch))
    assert torch.isfinite(ret['loss']) and disp == {}
    assert set(tb) == {'loss_rpn', 'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir', 'rpn_loss'}
    ret['loss'].backward()
    for name, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    assert all(h.conv_cls.weight.grad.abs().max() > 0 for h in model.dense_head.rpn_heads)
    model.eval()
    with torch.no_grad():
        pred_dicts, recall = model(dict(batch))
    assert len(pred_dicts) == B and set(pred_dicts[0]) == {'pred_boxes', 'pred_scores', 'pred_labels'}
    assert all(d['pred_boxes'].shape == (len(d['pred_scores']), 7) and d['pred_labels'].dtype == torch.int64 for d in pred_dicts)
    assert all(((d['pred_labels'] >= 1) & (d['pred_labels'] <= 3)).all() for d in pred_dicts)
    assert set(recall) == {'gt', 'roi_0.3', 'rcnn_0.3', 'roi_0.5', 'rcnn_0.5', 'roi_0.7', 'rcnn_0.7'}
    fresh = SECONDNet(to_attr(cfg), 3, ds).cuda()
    fresh.load_state_dict({k: v.clone() for k, v in model.state_dict().items()}, strict=True)
