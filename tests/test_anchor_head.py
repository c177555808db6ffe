"""The anchor head (AnchorGenerator, AxisAlignedTargetAssigner, AnchorHeadSingle) and the PointPillar detector against
tests/golden/anchor_head.npz, the reference's own output on CPU tensors (tests/golden/make_anchor_head_golden.py).

CPU part: the symbols, argument validation, every NotImplementedError of the contract, the no-CPU-path error, the
state-dict keys, the anchors bit for bit, and the numpy restatement of the contract (tests/golden/anchor_head_restatement.py)
against the fixture.  GPU part: the kernels against the same fixture.

Tolerances.  Labels, weights and positives counts are integers: equal.  Target columns 0-2 and 6 are float32 operations in
the reference's order: bit-identical; columns 3-5 are a correctly rounded log against torch's 1-ulp log: one float32 ulp.
Decoding: centres and heading are float32 operations (bit-identical without the direction classifier, 2 ulp with it, as the
issue sets); sizes are exp good to 1 ulp times the anchor's size: 2 ulp.  Losses within 2e-5 absolute, gradients within
2e-5 of the largest reference gradient magnitude (the bound the CenterPoint and RoI tests use)."""
import ctypes
import gc
import json
import os
import sys

import numpy as np
import pytest
import torch

from pdanet_amd import _lib, anchor_head as ah, build
from pdanet_amd.config import to_attr
from pdanet_amd.pointpillar import PointPillar

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import anchor_head_restatement as rs  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "anchor_head.npz")
G = np.load(FIXTURE)
CONFIGS = json.loads(str(G['configs']))
B = 2
BATCHES = [(c, t) for c in 'ab' for t in 'xyz']
LOSS_TOL = 2e-5


def ulps(a, b):
    """Distance in float32 steps."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)

    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(a) - ordered(b))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def make_head(c, input_channels=16, **over):
    cfg = CONFIGS[c]
    pcr, vs = np.array(cfg['point_cloud_range'], np.float64), np.array(cfg['voxel_size'], np.float64)
    grid = np.round((pcr[3:] - pcr[:3]) / vs).astype(np.int64)
    head_cfg = json.loads(json.dumps(cfg['head']))
    for path, value in over.items():
        node = head_cfg
        keys = path.split('__')
        for k in keys[:-1]:
            node = node[k]
        node[keys[-1]] = value
    return ah.AnchorHeadSingle(model_cfg=to_attr(head_cfg), input_channels=input_channels, num_class=cfg['num_class'],
                               class_names=cfg['class_names'], grid_size=grid, point_cloud_range=pcr,
                               predict_boxes_when_training=False)


def class_arrays(c):
    cfg = CONFIGS[c]
    gen = cfg['head']['ANCHOR_GENERATOR_CONFIG']
    return ([cfg['class_names'].index(g['class_name']) + 1 for g in gen], [g['matched_threshold'] for g in gen],
            [g['unmatched_threshold'] for g in gen], [int(v) for v in G[c + '_counts']])


def preds_of(c):
    d = G[c + '_dir_cls_preds'].astype(np.float32) if c + '_dir_cls_preds' in G else None
    return G[c + '_cls_preds'].astype(np.float32), G[c + '_box_preds'].astype(np.float32), d


def check_targets(c, t, labels, targets, weights, num_pos):
    p = c + t + '_'
    ref_l, ref_t, ref_w = G[p + 'box_cls_labels'], G[p + 'box_reg_targets'], G[p + 'reg_weights']
    assert labels.dtype == np.int32 and labels.shape == ref_l.shape          # no anchor is left out
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


NAMES = ["pda_anchor_assign_targets", "pda_anchor_loss_blocks", "pda_anchor_loss", "pda_anchor_decode", "pda_pillar_features"]


def test_symbols_exported(lib):
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.SIGNATURES


def test_fixture_is_small_and_covers_the_cases():
    assert os.path.getsize(FIXTURE) < 1 << 20
    assert G['a_table'].shape == (7680, 7) and G['b_table'].shape == (3800, 7) and 3800 % 64 and 3800 % 256
    for c in 'ab':
        gt = G[c + 'x_gt_boxes'][0]
        assert bits_equal(gt[0], gt[1])                                        # two identical boxes
        zero = ~gt.any(axis=1)
        assert zero[6] and not zero[7] and zero[-3:].all()                      # an interior zero row, trailing zero rows
        assert abs(gt[5, 6]) > np.pi / 4 and abs(gt[5, 6]) < np.pi / 2                         # a heading past pi / 4
        lab, mx, umx, counts = class_arrays(c)
        slots = sum(counts)
        cls_of = np.concatenate([np.full(k, i) for i, k in enumerate(counts)])[np.arange(len(G[c + '_table'])) % slots]
        iou = np.zeros((len(cls_of), gt.shape[0]), np.float32)
        for i in range(len(lab)):
            iou[cls_of == i] = G['%sx_iou_%d' % (c, i)]
        labels = G[c + 'x_box_cls_labels'][0]
        assert iou[:, 4].max() == 0                                             # a box that overlaps no anchor
        sq = iou[:, 2] * (np.array(lab)[cls_of] == gt[2, 7])
        assert (sq == sq.max()).sum() >= 2 and (labels[sq == sq.max()] > 0).all()      # a tie for the column maximum
        sm = iou[:, 3] * (np.array(lab)[cls_of] == gt[3, 7])
        un = np.array(umx)[cls_of][sm == sm.max()]
        assert (sm.max() < un).all() and (labels[sm == sm.max()] > 0).all()     # a forced positive below unmatched
        assert (labels < 0).any() and (G[c + 'z_box_cls_labels'] == 0).all()
        assert (G[c + 'y_box_cls_labels'][0] == 0).all() and (G[c + 'y_box_cls_labels'][1] > 0).any()


def test_argument_validation_without_gpu(lib):
    i64, d = ctypes.c_int64, ctypes.c_double
    one = (ctypes.c_int32 * 2)(1, 2)
    thr = (ctypes.c_float * 2)(0.6, 0.5)
    cnt = (ctypes.c_int32 * 2)(2, 2)
    assign = lambda cols, b, m, n, n_cls, lab=one, count=cnt: lib.pda_anchor_assign_targets(
        None, cols, b, m, None, n, n_cls, lab, thr, thr, count, None, None, None, None, None, None)
    assert assign(10, 1, 4, 8, 2) == 1 and b"gt_cols" in lib.pda_last_error()
    assert assign(8, -1, 4, 8, 2) == 1
    assert assign(8, 1, 4, 8, 0) == 1 and b"n_cls" in lib.pda_last_error()
    assert assign(8, 0, 4, 8, 2) == 0                                           # the empty problem
    assert assign(8, 1, 4, 8, 2, lab=(ctypes.c_int32 * 2)(1, 1)) == 1 and b"share label" in lib.pda_last_error()
    assert assign(8, 1, 4, 8, 2, count=(ctypes.c_int32 * 2)(40, 40)) == 1 and b"per location" in lib.pda_last_error()
    assert assign(8, 1, 4, 6, 2) == 1 and b"multiple" in lib.pda_last_error()
    assert assign(8, 1, 4, 8, 2) == 1 and b"null" in lib.pda_last_error()
    assert lib.pda_anchor_loss_blocks(i64(0)) == 0 and lib.pda_anchor_loss_blocks(i64(1)) == 1
    assert lib.pda_anchor_loss_blocks(i64(1025)) == 2 and lib.pda_anchor_loss_blocks(i64(1 << 30)) == 2048
    w = (ctypes.c_float * 7)(*[1.0] * 7)
    loss = lambda b, n, nc: lib.pda_anchor_loss(None, None, None, None, None, None, None, b, n, nc, 2, w, d(1), d(2), d(0.2),
                                                d(0.78), None, None, None, None, None, None)
    assert loss(0, 8, 3) == 1 and loss(1, 8, 0) == 1 and b"num_class" in lib.pda_last_error()
    assert loss(1, 8, 3) == 1 and b"null" in lib.pda_last_error()
    dec = lambda b, n: lib.pda_anchor_decode(None, None, None, b, n, 2, d(0.78), d(0.0), None, None)
    assert dec(-1, 8) == 1 and dec(0, 8) == 0 and dec(1, 8) == 1 and b"null" in lib.pda_last_error()


def test_out_of_contract_is_not_implemented():
    for over in ({'TARGET_ASSIGNER_CONFIG__POS_FRACTION': 0.5}, {'TARGET_ASSIGNER_CONFIG__NORM_BY_NUM_EXAMPLES': True},
                 {'TARGET_ASSIGNER_CONFIG__MATCH_HEIGHT': True}, {'TARGET_ASSIGNER_CONFIG__NAME': 'ATSS'},
                 {'USE_MULTIHEAD': True}, {'TARGET_ASSIGNER_CONFIG__BOX_CODER_CONFIG': {'encode_angle_by_sincos': True}},
                 {'TARGET_ASSIGNER_CONFIG__BOX_CODER_CONFIG': {'code_size': 9}}):
        with pytest.raises(NotImplementedError):
            make_head('a', **over)
    gen = json.loads(json.dumps(CONFIGS['a']['head']['ANCHOR_GENERATOR_CONFIG']))
    gen[1]['feature_map_stride'] = 4
    with pytest.raises(NotImplementedError, match="feature_map_stride"):
        make_head('a', ANCHOR_GENERATOR_CONFIG=gen)
    head = make_head('a')
    with pytest.raises(NotImplementedError, match="7 \\+ 1"):
        head.target_assigner.assign_targets(head.anchors, torch.zeros(1, 4, 10))


def test_no_cpu_path():
    head = make_head('a')
    with pytest.raises(RuntimeError, match="no CPU path"):
        head.assign_targets(torch.zeros(1, 4, 8))
    cls, box, d = (torch.from_numpy(v) for v in preds_of('a'))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ah.anchor_decode(box, d, torch.from_numpy(G['a_table']))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ah.anchor_loss(cls, box, d, torch.from_numpy(G['ax_box_cls_labels']), torch.from_numpy(G['ax_box_reg_targets']),
                       torch.zeros(2, dtype=torch.int32), torch.from_numpy(G['a_table']), 3, [1.0] * 7, 1.0, 2.0, 0.2, 0.78539)


def test_state_dict_keys_and_anchors_are_the_references():
    for c in 'ab':
        head = make_head(c)
        assert list(head.state_dict().keys()) == [str(k) for k in G['keys_' + c]]
        head.load_state_dict({k: v.clone() for k, v in head.state_dict().items()}, strict=True)
        assert len(head.anchors) == len(CONFIGS[c]['head']['ANCHOR_GENERATOR_CONFIG'])
        for i, a in enumerate(head.anchors):
            assert bits_equal(a.numpy(), G['%s_anchors_%d' % (c, i)]), "anchors of class %d" % i
        table, counts = ah.anchor_table(head.anchors)
        assert bits_equal(table.numpy(), G[c + '_table']) and counts == [int(v) for v in G[c + '_counts']]
        assert head.num_anchors_per_location * np.prod(head.anchors[0].shape[1:3]) == len(table)
    assert make_head('b').conv_dir_cls is None and make_head('a').conv_dir_cls is not None
    assert abs(float(make_head('a').conv_cls.bias[0]) + np.log(99.0)) < 1e-6


@pytest.mark.parametrize("c", "ab")
def test_restatement_iou(c):
    lab, mx, umx, counts = class_arrays(c)
    table, gt = G[c + '_table'], G[c + 'x_gt_boxes'][0]
    slots = sum(counts)
    cls_of = np.concatenate([np.full(k, i) for i, k in enumerate(counts)])[np.arange(len(table)) % slots]
    for i in range(len(lab)):
        assert bits_equal(rs.nearest_bev_iou(table[cls_of == i], gt[:, :7]), G['%sx_iou_%d' % (c, i)]), "IoU of class %d" % i


@pytest.mark.parametrize("c,t", BATCHES)
def test_restatement_targets(c, t):
    check_targets(c, t, *rs.assign_targets(G[c + t + '_gt_boxes'], G[c + '_table'], *class_arrays(c)))


@pytest.mark.parametrize("c,t", BATCHES)
def test_restatement_losses(c, t):
    cfg, p = CONFIGS[c]['head'], c + t + '_'
    w = cfg['LOSS_CONFIG']['LOSS_WEIGHTS']
    cls, box, d = preds_of(c)
    got = rs.losses(cls, box, d, G[p + 'box_cls_labels'], G[p + 'box_reg_targets'], G[c + '_table'], CONFIGS[c]['num_class'],
                    w['code_weights'], w['cls_weight'], w['loc_weight'], w['dir_weight'], cfg.get('DIR_OFFSET', 0.0))
    assert np.abs(got - G[p + 'losses']).max() <= LOSS_TOL


def check_decode(c, boxes):
    ref = G[c + '_batch_box_preds']
    assert boxes.shape == ref.shape
    assert bits_equal(boxes[..., :3], ref[..., :3]), "centres"
    assert ulps(boxes[..., 3:6], ref[..., 3:6]).max() <= 2, "sizes"
    if c + '_dir_cls_preds' in G:
        assert ulps(boxes[..., 6], ref[..., 6]).max() <= 2, "heading behind the direction classifier"
    else:
        assert bits_equal(boxes[..., 6], ref[..., 6]), "heading"


@pytest.mark.parametrize("c", "ab")
def test_restatement_decode(c):
    cls, box, d = preds_of(c)
    cfg = CONFIGS[c]['head']
    check_decode(c, rs.decode(box, d, G[c + '_table'], cfg.get('DIR_OFFSET', 0.0), cfg.get('DIR_LIMIT_OFFSET', 0.0)))


def test_pointpillar_refuses_other_modules():
    cfg = pointpillar_cfg()
    cfg['DENSE_HEAD']['NAME'] = 'AnchorHeadMulti'
    with pytest.raises(NotImplementedError):
        PointPillar(to_attr(cfg), 3, DATASET)
    cfg = pointpillar_cfg()
    cfg['VFE']['NAME'] = 'MeanVFE'
    with pytest.raises(NotImplementedError):
        PointPillar(to_attr(cfg), 3, DATASET)


def pointpillar_cfg():
    return {'NAME': 'PointPillar',
            'VFE': {'NAME': 'PillarVFE', 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'USE_NORM': True, 'NUM_FILTERS': [32]},
            'MAP_TO_BEV': {'NAME': 'PointPillarScatter', 'NUM_BEV_FEATURES': 32},
            'BACKBONE_2D': {'NAME': 'BaseBEVBackbone', 'LAYER_NUMS': [1, 1], 'LAYER_STRIDES': [2, 2], 'NUM_FILTERS': [32, 64],
                            'UPSAMPLE_STRIDES': [1, 2], 'NUM_UPSAMPLE_FILTERS': [32, 32]},
            'DENSE_HEAD': dict(json.loads(json.dumps(CONFIGS['a']['head'])), NAME='AnchorHeadSingle'),
            'POST_PROCESSING': {'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'SCORE_THRESH': 0.1, 'OUTPUT_RAW_SCORE': False,
                                'NMS_CONFIG': {'MULTI_CLASSES_NMS': False, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.01,
                                               'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 500}}}


DATASET = {'class_names': CONFIGS['a']['class_names'], 'point_cloud_range': CONFIGS['a']['point_cloud_range'],
           'voxel_size': CONFIGS['a']['voxel_size'], 'num_point_features': 4}


def test_pointpillar_state_dict_is_unchanged():
    """Names and shapes in order, as recorded from the commit before the detectors were folded onto one base class."""
    with open(os.path.join(HERE, "golden", "pillar_detector_state_dicts.json")) as f:
        ref = json.load(f)['PointPillar']
    assert [[k, list(v.shape)] for k, v in PointPillar(to_attr(pointpillar_cfg()), 3, DATASET).state_dict().items()] == ref


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
    """m = 70 boxes of one class on configuration b: more than a wave and more than one 64-row tile; against the restatement."""
    rng = np.random.default_rng(7)
    cfg = CONFIGS['b']
    pcr = cfg['point_cloud_range']
    m = 70
    gt = np.zeros((1, m, 8), np.float32)
    gt[0, :, 0] = rng.uniform(pcr[0], pcr[3], m)
    gt[0, :, 1] = rng.uniform(pcr[1], pcr[4], m)
    gt[0, :, 2] = -1.0
    gt[0, :, 3:6] = np.array([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.2, (m, 3))
    gt[0, :, 6] = rng.uniform(-3, 3, m)
    gt[0, :, 7] = 1
    gt[0, 20] = 0                                                              # an interior zero row
    head = make_head('b').cuda()
    _, (labels, targets, weights, num_pos) = run_targets(head, dev(gt))
    ref = rs.assign_targets(gt, G['b_table'], *class_arrays('b'))
    assert np.array_equal(labels, ref[0]) and np.array_equal(num_pos, ref[3]) and bits_equal(weights, ref[2])
    assert (labels > 0).sum() > 64 and (labels < 0).any()
    # the last tile's boxes are matched too
    assert bits_equal(targets[..., [0, 1, 2, 6]], ref[1][..., [0, 1, 2, 6]]) and ulps(targets[..., 3:6], ref[1][..., 3:6]).max() <= 1


def head_loss(head, c, t):
    cls, box, d = preds_of(c)
    H, W = head.anchors[0].shape[1:3]
    leaves = {'cls_preds': dev(cls.reshape(B, H, W, -1)).requires_grad_(True), 'box_preds': dev(box.reshape(B, H, W, -1)).requires_grad_(True)}
    if d is not None:
        leaves['dir_cls_preds'] = dev(d.reshape(B, H, W, -1)).requires_grad_(True)
    head.forward_ret_dict = dict(leaves, **head.assign_targets(dev(G[c + t + '_gt_boxes'])))
    loss, tb = head.get_loss()
    return loss, tb, leaves


def check_losses(c, t, tb, grads):
    p = c + t + '_'
    ref = G[p + 'losses']
    keys = ['rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir', 'rpn_loss']
    has_dir = c + '_dir_cls_preds' in G
    assert set(tb) == set(keys if has_dir else [k for k in keys if k != 'rpn_loss_dir'])
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 and v.is_cuda for v in tb.values())
    d_loss = [abs(float(tb[k]) - float(ref[i])) for i, k in enumerate(keys) if k in tb]
    refs = {k: G[p + 'g_' + k] for k in grads}
    scale = max(float(np.abs(v).max()) for v in refs.values())
    d_g = max(float(np.abs(grads[k].reshape(refs[k].shape).astype(np.float64) - refs[k]).max()) for k in grads)
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
    check_losses(c, t, tb, {k: v.grad.cpu().numpy() for k, v in leaves.items()})
    assert float(loss.detach()) == float(tb['rpn_loss'])
    assert torch.equal(head.forward_ret_dict['box_cls_labels'], before), "the labels were rewritten"


def loss_case(n):
    """One scene of n anchors of one class, two direction bins: logits around -4, about 5 % ignored anchors, up to five
    positives (the first and the last anchor among them), one of them with a NaN regression target."""
    rng = np.random.default_rng(n)
    table = np.zeros((n, 7), np.float32)
    table[:, :2] = rng.uniform(-40, 40, (n, 2))
    table[:, 3:6] = (3.9, 1.6, 1.56)
    table[:, 6] = rng.choice(np.array([0.0, 1.57], np.float32), n)
    cls = rng.normal(-4.0, 1.0, (1, n, 1)).astype(np.float32)
    box = rng.normal(0.0, 0.3, (1, n, 7)).astype(np.float32)
    dirs = rng.normal(0.0, 1.0, (1, n, 2)).astype(np.float32)
    labels = np.where(rng.random((1, n)) < 0.05, -1, 0).astype(np.int32)
    pos = np.unique(np.linspace(0, n - 1, min(n, 5)).astype(np.int64))
    labels[0, pos] = 1
    targets = np.zeros((1, n, 7), np.float32)
    targets[0, pos] = rng.normal(0.0, 0.3, (len(pos), 7))
    targets[0, pos[0], 2] = np.nan
    return cls, box, dirs, labels, targets, np.array([len(pos)], np.int32), table


LOSS_CASE_WEIGHTS = dict(num_class=1, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], cls_weight=1.0, loc_weight=2.0,
                         dir_weight=0.2, dir_offset=0.78539)


@gpu
@pytest.mark.parametrize("n,blocks", [(1, 1), (1025, 2), (2097153, 2048)])
def test_gpu_anchor_loss_at_the_block_boundaries(n, blocks):
    """The sizes at which the shared partial sums (csrc/loss_sums.h) can go wrong: one anchor; one full workgroup of 1024
    and one anchor; one anchor past the 2048-workgroup cap, where the grid-stride loop wraps.  Against the float64
    restatement, within test_gpu_losses' bound."""
    assert _lib.load().pda_anchor_loss_blocks(n) == blocks
    cls, box, dirs, labels, targets, num_pos, table = loss_case(n)
    ref = rs.losses(cls, box, dirs, labels, targets, table, **LOSS_CASE_WEIGHTS)
    leaves = [dev(v).requires_grad_(True) for v in (cls, box, dirs)]
    loss, out = ah.anchor_loss(*leaves, dev(labels), dev(targets), dev(num_pos), dev(table), **LOSS_CASE_WEIGHTS)
    loss.backward()
    d_loss = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    print("anchor n", n, "losses", ref, "diff", ["%.3g" % v for v in d_loss])
    assert d_loss.max() <= LOSS_TOL
    assert float(loss.detach()) == float(out[3])
    g_box = leaves[1].grad.cpu().numpy()
    assert all(bool(torch.isfinite(v.grad).all()) for v in leaves) and g_box[0, 0, 2] == 0      # the NaN target
    assert g_box[0, 0, [0, 1, 3, 4, 5, 6]].all() and not g_box[labels <= 0].any()


@gpu
@pytest.mark.parametrize("c", "ab")
def test_gpu_decode(c):
    head = make_head(c).cuda().eval()
    cls, box, d = preds_of(c)
    H, W = head.anchors[0].shape[1:3]
    bc, bb = head.generate_predicted_boxes(B, dev(cls.reshape(B, H, W, -1)), dev(box.reshape(B, H, W, -1)),
                                           None if d is None else dev(d.reshape(B, H, W, -1)))
    assert bits_equal(bc.cpu().numpy(), cls)
    check_decode(c, bb.cpu().numpy())


def selection_head(c):
    """A head whose 1x1 convolutions copy channels of the input, so that a forward on the fixture's predictions laid out as
    a (B, C, H, W) map reproduces them exactly (1 * x plus zeros)."""
    cls, box, d = preds_of(c)
    parts = [cls, box] + ([d] if d is not None else [])
    head = make_head(c)
    H, W = head.anchors[0].shape[1:3]
    maps = [p.reshape(B, H, W, -1).transpose(0, 3, 1, 2) for p in parts]
    channels = [m.shape[1] for m in maps]
    head = make_head(c, input_channels=sum(channels)).cuda().train()
    convs = [head.conv_cls, head.conv_box] + ([head.conv_dir_cls] if d is not None else [])
    off = 0
    with torch.no_grad():
        for conv, n in zip(convs, channels):
            conv.weight.zero_()
            conv.bias.zero_()
            conv.weight[torch.arange(n), off + torch.arange(n), 0, 0] = 1.0
            off += n
    return head, dev(np.concatenate(maps, axis=1)), convs


@gpu
def test_gpu_backward_reaches_the_convolutions():
    head, feats, convs = selection_head('a')
    head({'spatial_features_2d': feats, 'gt_boxes': dev(G['ax_gt_boxes']), 'batch_size': B})
    loss, tb = head.get_loss()
    loss.backward()
    for conv in convs:
        assert conv.weight.grad is not None and torch.isfinite(conv.weight.grad).all() and conv.weight.grad.abs().max() > 0
        assert conv.bias.grad.abs().max() > 0
    assert np.abs(np.array([float(tb[k]) for k in ('rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir', 'rpn_loss')])
                  - G['ax_losses']).max() <= LOSS_TOL


@gpu
def test_gpu_no_host_read_and_graph_replay():
    """forward + get_loss + backward read nothing back (sync debug mode 'error'), are captured once and replayed on a second
    batch: the replay gives that batch's fixture losses."""
    head, feats, convs = selection_head('a')
    params = [p for conv in convs for p in (conv.weight, conv.bias)]
    gt = dev(G['ax_gt_boxes'])

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
    eager = [float(tb[k]) for k in ('rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir', 'rpn_loss')]
    assert np.abs(np.array(eager) - G['ax_losses']).max() <= LOSS_TOL
    del tb, grads
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    # nothing of an earlier iteration may be alive at the capture: forward_ret_dict holds the warm-up's predictions, whose
    # autograd graph references the parameters about to be captured ("Known gaps")
    head.forward_ret_dict.clear()
    gc.collect()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tb_g, grads_g = step()
    gt.copy_(dev(G['ay_gt_boxes']))                            # the second batch, into the captured input
    graph.replay()
    torch.cuda.synchronize()
    replay = [float(tb_g[k]) for k in ('rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir', 'rpn_loss')]
    assert np.abs(np.array(replay) - G['ay_losses']).max() <= LOSS_TOL
    assert all(torch.isfinite(g).all() for g in grads_g)
    assert np.array_equal(head.forward_ret_dict['box_cls_labels'].cpu().numpy(), G['ay_box_cls_labels'])


@gpu
def test_gpu_pointpillar_train_and_eval():
    from pdanet_amd.voxel_utils import VoxelGenerator, collate_voxels
    cfg = CONFIGS['a']
    torch.manual_seed(3)
    model = PointPillar(to_attr(pointpillar_cfg()), 3, DATASET).cuda()
    rng = np.random.default_rng(5)
    pcr = np.array(cfg['point_cloud_range'])
    counts = [1500, 900]                                       # a ragged scene pair
    pts = np.concatenate([np.concatenate([rng.uniform(pcr[:3], pcr[3:], (n, 3)), rng.random((n, 1))], axis=1) for n in counts])
    offs = torch.tensor([0, counts[0], sum(counts)], dtype=torch.int64).cuda()
    gen = VoxelGenerator(cfg['voxel_size'], cfg['point_cloud_range'], 4, 32, 2000)
    voxels, coords, num_points = collate_voxels(*gen.generate_batch((dev(pts.astype(np.float32)), offs, max(counts))))
    assert voxels.shape[0] == coords.shape[0] == num_points.shape[0] and coords.shape[1] == 4 and (num_points > 0).all()
    assert int(coords[:, 0].max()) == 1 and voxels.shape[1:] == (32, 4)
    batch = {'voxels': voxels, 'voxel_coords': coords, 'voxel_num_points': num_points, 'gt_boxes': dev(G['ax_gt_boxes']),
             'batch_size': B}
    model.train()
    ret, tb, disp = model(dict(batch))
    assert torch.isfinite(ret['loss']) and disp == {}
    assert set(tb) == {'loss_rpn', 'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir', 'rpn_loss'}
    ret['loss'].backward()
    for name, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    model.eval()
    with torch.no_grad():
        pred_dicts, recall = model(dict(batch))
    assert len(pred_dicts) == B and set(pred_dicts[0]) == {'pred_boxes', 'pred_scores', 'pred_labels'}
    assert set(recall) == {'gt', 'roi_0.3', 'rcnn_0.3', 'roi_0.5', 'rcnn_0.5', 'roi_0.7', 'rcnn_0.7'}
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    fresh = PointPillar(to_attr(pointpillar_cfg()), 3, DATASET).cuda()
    fresh.load_state_dict(sd, strict=True)
    assert all(k.split('.')[0] in ('vfe', 'map_to_bev_module', 'backbone_2d', 'dense_head') for k in sd)
