"""The CenterPoint pillar tail (PointPillarScatter, CenterHead) against tests/golden/center_head.npz, the reference's own
output on CPU tensors (tests/golden/make_center_head_golden.py).

CPU part: the symbols, argument validation, the no-CPU-path error, the state-dict keys, and the numpy restatement of the
contract (tests/golden/center_head_restatement.py) against the fixture.  GPU part: the kernels against the same fixture.

Tolerances.  One float32 ulp for log / cos / sin and the Gaussian: a float64 evaluation good to 1 ulp leaves at most that
after one rounding against torch's / numpy's own 1-ulp float32 and correctly rounded float64 results.  Two ulp for xs, ys,
exp and atan2 of the decoding (the issue's bound) and for the scores: expf good to 1 ulp, then one addition and one division,
against torch's sigmoid built the same way.  Losses within 2e-5 absolute, gradients within 2e-5 of the largest reference
gradient magnitude.  The regression loss with NaN targets is compared with the reference run on targets whose NaN entries
are replaced by the prediction at their cell (the reference itself returns NaN there; see the maker's docstring)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from pdanet_amd import _lib, build, centernet_utils as cu, model_nms_utils
from pdanet_amd.base_bev_backbone import BaseBEVBackbone
from pdanet_amd.center_head import CenterHead, SeparateHead  # noqa: F401
from pdanet_amd.centerpoint import CenterPoint
from pdanet_amd.config import to_attr
from pdanet_amd.pointpillar_scatter import PointPillarScatter, pillar_scatter

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import center_head_restatement as rs  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "center_head.npz"))
CONFIGS = json.loads(str(G['configs']))
CLASS_NAMES = [str(c) for c in G['class_names']]
H, W = (int(v) for v in G['map_hw'])
B = 2
BATCHES = [(c, t) for c in 'ab' for t in 'xyz']
LOSS_TOL = 2e-5


def ulps(a, b):
    """Distance in float32 steps; equal infinities and NaN against NaN count as 0."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)

    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(ordered(a) - ordered(b))
    return np.where(np.isnan(a) & np.isnan(b), 0, d)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def kept_gt(gt):
    """The rows generate_recall_record keeps: each scene up to its last row with a non-zero sum (at least one)."""
    total = 0
    for rows in gt:
        nz = np.nonzero(~(np.nan_to_num(rows, nan=1.0).sum(-1) == 0))[0]
        total += int(nz[-1]) + 1 if len(nz) else 1
    return total


def n_heads(c):
    return len(CONFIGS[c]['head']['CLASS_NAMES_EACH_HEAD'])


def preds_of(c, h):
    keys = ['hm'] + list(CONFIGS[c]['head']['SEPARATE_HEAD_CFG']['HEAD_DICT'])
    return {k: G['%s_p%d_%s' % (c, h, k)].astype(np.float32) for k in keys}


def make_head(c, input_channels=16):
    cfg = CONFIGS[c]
    pcr, vs = np.array(cfg['point_cloud_range']), np.array(cfg['voxel_size'])
    grid = np.round((pcr[3:] - pcr[:3]) / vs).astype(np.int64)
    return CenterHead(model_cfg=to_attr(cfg['head']), input_channels=input_channels, num_class=3, class_names=CLASS_NAMES,
                      grid_size=grid, point_cloud_range=pcr, voxel_size=cfg['voxel_size'], predict_boxes_when_training=False)


def check_targets(got, c, t):
    """got: per head (heatmaps, target_boxes, inds, masks) as numpy.  Returns the heat-map cells that are not bit-identical."""
    p = c + t + '_'
    off = 0
    for h in range(n_heads(c)):
        hm, tb, inds, masks = got[h]
        ref_hm, ref_tb = G['%st%d_heatmaps' % (p, h)], G['%st%d_target_boxes' % (p, h)]
        assert np.array_equal(inds, G['%st%d_inds' % (p, h)]) and np.array_equal(masks, G['%st%d_masks' % (p, h)])
        assert inds.dtype == np.int64 and masks.dtype == np.int64
        assert bits_equal(tb[..., 0:3], ref_tb[..., 0:3]), "centre offset / z"
        assert bits_equal(tb[..., 8:], ref_tb[..., 8:]), "extra columns"
        assert ulps(tb[..., 3:8], ref_tb[..., 3:8]).max() <= 1, "log / cos / sin"
        assert np.array_equal(hm != 0, ref_hm != 0), "the set of non-zero heat-map cells"
        d = ulps(hm, ref_hm)
        assert d.max() <= 1, "heat map"
        off += int((d != 0).sum())
    return off


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


NAMES = ["pda_pillar_scatter_fwd", "pda_pillar_scatter_bwd", "pda_center_assign_targets", "pda_center_focal_blocks",
         "pda_center_focal_loss", "pda_center_scale", "pda_center_reg_loss", "pda_center_reg_loss_grad", "pda_center_decode"]


def test_symbols_exported(lib):
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.SIGNATURES


def test_argument_validation_without_gpu(lib):
    i64, f = ctypes.c_int64, ctypes.c_float
    # sizes first, then the empty problem, then pointers
    assert lib.pda_pillar_scatter_fwd(None, None, None, i64(-1), 4, 1, 2, 2, None, None) == 1
    assert lib.pda_pillar_scatter_fwd(None, None, None, i64(0), 4, 1, 2, 2, None, None) == 0
    assert lib.pda_pillar_scatter_fwd(None, None, None, i64(5), 4, 1, 2, 2, None, None) == 1 and b"null" in lib.pda_last_error()
    assert lib.pda_pillar_scatter_bwd(None, None, None, i64(0), 4, 1, 2, 2, None, None) == 0
    assert lib.pda_pillar_scatter_bwd(None, None, None, i64(5), 4, 1, 2, 2, None, None) == 1
    d = [ctypes.c_double(v) for v in (0.0, 0.0, 0.1, 0.1, 1.0, 0.1)]
    assert lib.pda_center_assign_targets(None, 7, 1, 4, 3, 1, None, None, None, 8, 8, 16, *d, 2, None, None, None, None, None) == 1
    assert b"gt_cols" in lib.pda_last_error()
    assert lib.pda_center_assign_targets(None, 8, 1, 4, 3, 1, None, None, None, 8, 8, 4096, *d, 2, None, None, None, None, None) == 1
    assert b"max_objs" in lib.pda_last_error()
    assert lib.pda_center_assign_targets(None, 8, 1, 4, 3, 9, None, None, None, 8, 8, 16, *d, 2, None, None, None, None, None) == 1
    assert lib.pda_center_assign_targets(None, 8, 0, 4, 3, 1, None, None, None, 8, 8, 16, *d, 2, None, None, None, None, None) == 0
    assert lib.pda_center_assign_targets(None, 8, 1, 4, 3, 1, None, None, None, 8, 8, 16, *d, 2, None, None, None, None, None) == 1
    assert b"null" in lib.pda_last_error()
    assert lib.pda_center_focal_blocks(i64(0)) == 0 and lib.pda_center_focal_blocks(i64(1)) == 1
    assert lib.pda_center_focal_blocks(i64(2048)) == 1 and lib.pda_center_focal_blocks(i64(2049)) == 2
    assert lib.pda_center_focal_blocks(i64(1 << 30)) == 1024
    assert lib.pda_center_focal_loss(None, None, i64(-1), None, None, None, None) == 1
    assert lib.pda_center_focal_loss(None, None, i64(0), None, None, None, None) == 0
    assert lib.pda_center_focal_loss(None, None, i64(8), None, None, None, None) == 1 and b"null" in lib.pda_last_error()
    assert lib.pda_center_scale(None, None, None, f(1), i64(0), None, None) == 0
    assert lib.pda_center_scale(None, None, None, f(1), i64(4), None, None) == 1
    assert lib.pda_center_reg_loss(None, None, 0, None, None, None, None, f(1), 1, 1, i64(4), None, None) == 1
    assert b"n_maps" in lib.pda_last_error()
    assert lib.pda_center_reg_loss(None, None, 2, None, None, None, None, f(1), 0, 8, i64(4), None, None) == 0
    assert lib.pda_center_reg_loss(None, None, 2, None, None, None, None, f(1), 2, 8, i64(4), None, None) == 1
    assert lib.pda_center_reg_loss_grad(None, None, 2, None, None, None, None, f(1), 2, 0, i64(4), None, None, None, None) == 0
    dd = [ctypes.c_double(v) for v in (1.0, 0.1, 0.1, 0.0, 0.0)]
    assert lib.pda_center_decode(None, None, None, None, None, None, None, 1, 4, 8, 8, 0, None, *dd, None, 0, ctypes.c_double(0),
                                 None, None, None, None) == 1 and b"n_cls" in lib.pda_last_error()
    assert lib.pda_center_decode(None, None, None, None, None, None, None, 0, 4, 8, 8, 3, None, *dd, None, 0, ctypes.c_double(0),
                                 None, None, None, None) == 0
    assert lib.pda_center_decode(None, None, None, None, None, None, None, 1, 4, 8, 8, 3, None, *dd, None, 0, ctypes.c_double(0),
                                 None, None, None, None) == 1 and b"null" in lib.pda_last_error()


def test_no_cpu_path():
    feats, coords = torch.zeros(4, 8), torch.zeros(4, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pillar_scatter(feats, coords, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        PointPillarScatter({'NUM_BEV_FEATURES': 8}, (4, 4, 1))({'pillar_features': feats, 'voxel_coords': coords, 'batch_size': 1})
    head = make_head('a')
    with pytest.raises(RuntimeError, match="no CPU path"):
        head.assign_targets(torch.zeros(1, 4, 8), feature_map_size=(H, W))
    with pytest.raises(RuntimeError, match="no CPU path"):
        cu.focal_loss(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        cu.decode_topk({k: torch.from_numpy(v) for k, v in preds_of('a', 0).items()}, 8, [0, 1, 2], [0, 0], [1, 1], 1, [0] * 6)
    with pytest.raises(AssertionError):
        PointPillarScatter({'NUM_BEV_FEATURES': 8}, (4, 4, 2))


def test_circle_nms_is_not_implemented():
    cfg = json.loads(json.dumps(CONFIGS['a']['head']))
    cfg['POST_PROCESSING']['NMS_CONFIG']['NMS_TYPE'] = 'circle_nms'
    head = CenterHead(to_attr(cfg), 16, 3, CLASS_NAMES, [W, H, 1], CONFIGS['a']['point_cloud_range'], CONFIGS['a']['voxel_size'])
    with pytest.raises(NotImplementedError):
        head.generate_predicted_boxes(1, [])


def test_state_dict_keys_are_the_references():
    for c in 'ab':
        head = make_head(c)
        assert list(head.state_dict().keys()) == [str(k) for k in G['keys_' + c]]
        head.load_state_dict({k: v.clone() for k, v in head.state_dict().items()}, strict=True)
    bev = BaseBEVBackbone(to_attr(json.loads(str(G['bev_cfg']))), 64)
    assert list(bev.state_dict().keys()) == [str(k) for k in G['keys_bev']]
    assert bev.num_bev_features == 384
    assert list(PointPillarScatter(to_attr({'NUM_BEV_FEATURES': 64}), (W, H, 1)).state_dict().keys()) == []


def centerpoint_cfg():
    return {'NAME': 'CenterPoint',
            'VFE': {'NAME': 'DynPillarVFE', 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'USE_NORM': True, 'NUM_FILTERS': [32, 32]},
            'MAP_TO_BEV': {'NAME': 'PointPillarScatter', 'NUM_BEV_FEATURES': 32},
            'BACKBONE_2D': {'NAME': 'BaseBEVBackbone', 'LAYER_NUMS': [1, 1, 1], 'LAYER_STRIDES': [1, 2, 2], 'NUM_FILTERS': [32, 64, 64],
                            'UPSAMPLE_STRIDES': [1, 2, 4], 'NUM_UPSAMPLE_FILTERS': [32, 32, 32]},
            'DENSE_HEAD': dict(json.loads(json.dumps(CONFIGS['a']['head'])), NAME='CenterHead'),
            'POST_PROCESSING': {'RECALL_THRESH_LIST': [0.3, 0.5, 0.7]}}


DATASET = {'class_names': CLASS_NAMES, 'point_cloud_range': CONFIGS['a']['point_cloud_range'], 'voxel_size': CONFIGS['a']['voxel_size'],
           'num_point_features': 4}


def state_shapes(model):
    return [[k, list(v.shape)] for k, v in model.state_dict().items()]


def test_centerpoint_state_dict_is_unchanged():
    """Names and shapes in order, as recorded from the commit before the detectors were folded onto one base class."""
    with open(os.path.join(HERE, "golden", "pillar_detector_state_dicts.json")) as f:
        assert state_shapes(CenterPoint(to_attr(centerpoint_cfg()), 3, DATASET)) == json.load(f)['CenterPoint']


def test_centerpoint_refuses_other_modules():
    for key, name in (('DENSE_HEAD', 'AnchorHeadSingle'), ('VFE', 'MeanVFE'), ('BACKBONE_2D', 'BaseBEVResBackbone')):
        cfg = centerpoint_cfg()
        cfg[key]['NAME'] = name
        with pytest.raises(NotImplementedError) as err:
            CenterPoint(to_attr(cfg), 3, DATASET)
        assert str(err.value) == "%s.NAME %r (the sparse-conv backbones and other heads are not part of this project)" % (key, name)


@pytest.mark.parametrize("c,t", BATCHES)
def test_restatement_targets(c, t):
    cfg, tc = CONFIGS[c], CONFIGS[c]['head']['TARGET_ASSIGNER_CONFIG']
    got = rs.assign_targets(G[c + t + '_gt_boxes'], CLASS_NAMES, cfg['head']['CLASS_NAMES_EACH_HEAD'], (H, W), cfg['point_cloud_range'],
                            cfg['voxel_size'], tc['FEATURE_MAP_STRIDE'], tc['NUM_MAX_OBJS'], tc['GAUSSIAN_OVERLAP'], tc['MIN_RADIUS'])
    check_targets(got, c, t)


def check_loss(c, t, h, hm_loss, loc_loss, grads):
    """grads: dict name -> array; against the fixture within LOSS_TOL (absolute; gradients relative to the largest
    reference gradient).  Returns the differences."""
    p = c + t + '_'
    w = CONFIGS[c]['head']['LOSS_CONFIG']['LOSS_WEIGHTS']
    d_hm = abs(hm_loss - float(G['%sl%d_hm_loss' % (p, h)]))
    d_loc = abs(loc_loss - float(G['%sl%d_loc_loss' % (p, h)]))
    ref = {k: G['%sg%d_%s' % (p, h, k)] for k in grads}
    scale = max(float(np.abs(v).max()) for v in ref.values())
    d_g = max(float(np.abs(grads[k].astype(np.float64) - ref[k]).max()) for k in grads)
    print("loss", c, t, h, "hm %.3g loc %.3g grad %.3g of %.3g" % (d_hm, d_loc, d_g, scale), "cls_weight", w['cls_weight'])
    assert d_hm <= LOSS_TOL and d_loc <= LOSS_TOL
    assert d_g <= LOSS_TOL * scale
    return d_hm, d_loc, d_g / scale


@pytest.mark.parametrize("c,t", BATCHES)
def test_restatement_losses(c, t):
    p = c + t + '_'
    w = CONFIGS[c]['head']['LOSS_CONFIG']['LOSS_WEIGHTS']
    order = CONFIGS[c]['head']['SEPARATE_HEAD_CFG']['HEAD_ORDER']
    for h in range(n_heads(c)):
        pred = preds_of(c, h)
        hm_loss, g_hm = rs.focal_loss(pred['hm'], G['%st%d_heatmaps' % (p, h)])
        loc, g = rs.reg_loss([pred[k] for k in order], G['%st%d_masks' % (p, h)], G['%st%d_inds' % (p, h)],
                             G['%st%d_target_boxes' % (p, h)], w['code_weights'], w['loc_weight'])
        grads = dict(zip(order, g), hm=g_hm * w['cls_weight'])
        check_loss(c, t, h, hm_loss * w['cls_weight'], loc, grads)


def check_decode(c, h, ind, boxes, scores, labels):
    """The (B, K) outputs of the decoding against the reference's _topk and its masked, per-scene lists."""
    p = c + 'x_'
    cmap = np.array([CLASS_NAMES.index(n) for n in CONFIGS[c]['head']['CLASS_NAMES_EACH_HEAD'][h]])
    assert np.array_equal(ind % (H * W), G['%sd%d_topk_inds' % (p, h)]) and np.array_equal(ind // (H * W), G['%sd%d_topk_cls' % (p, h)])
    for s in range(B):
        keep = scores[s] > -np.inf
        rb, rsc, rl = (G['%sd%d_s%d_%s' % (p, h, s, k)] for k in ('boxes', 'scores', 'labels'))
        assert keep.sum() == len(rb) and 0 < keep.sum() < len(keep), "rows inside the limit range and above the threshold"
        assert np.array_equal(labels[s][keep], cmap[rl])
        b = boxes[s][keep]
        assert bits_equal(b[:, 2], rb[:, 2]) and bits_equal(b[:, 7:], rb[:, 7:]), "gathered columns"
        assert ulps(b[:, [0, 1, 3, 4, 5, 6]], rb[:, [0, 1, 3, 4, 5, 6]]).max() <= 2
        assert ulps(scores[s][keep], rsc).max() <= 2


@pytest.mark.parametrize("c", "ab")
def test_restatement_decode(c):
    cfg, pp = CONFIGS[c], CONFIGS[c]['head']['POST_PROCESSING']
    for h, names in enumerate(cfg['head']['CLASS_NAMES_EACH_HEAD']):
        pred = preds_of(c, h)
        if 'vel' not in cfg['head']['SEPARATE_HEAD_CFG']['HEAD_ORDER']:
            pred.pop('vel', None)
        out = rs.decode(pred, pp['MAX_OBJ_PER_SAMPLE'], [CLASS_NAMES.index(n) for n in names], cfg['point_cloud_range'],
                        cfg['voxel_size'], cfg['head']['TARGET_ASSIGNER_CONFIG']['FEATURE_MAP_STRIDE'],
                        pp['POST_CENTER_LIMIT_RANGE'], pp['SCORE_THRESH'])
        check_decode(c, h, *out)


def test_fixture_covers_the_cases():
    a, b = G['ax_gt_boxes'], G['bx_gt_boxes']
    assert int(G['ax_max_radius']) > 16 and np.isnan(b[..., 7:9]).any() and int(G['bx_n_nan_targets']) > 0
    assert np.isnan(float(G['bx_loss_nan'])) and np.isfinite(float(G['bx_loss']))
    assert (a[0, :, 3] == 0).sum() > (a[0, :, -1] == 0).sum()                 # a labelled box with dx = 0
    assert ((b[0, :, -1] >= 2).sum() > 8) and G['bx_t1_masks'].shape[1] == 8     # more than NUM_MAX_OBJS objects for head 1
    inds, masks = G['bx_t1_inds'][0], G['bx_t1_masks'][0]
    assert (inds[masks == 1] == 25 * W + 25).sum() == 3                        # three objects in one cell
    inds, masks = G['bx_t0_inds'][0], G['bx_t0_masks'][0]
    assert (inds[masks == 1] == 10 * W + 10).sum() == 2                        # two objects in one cell
    assert G['bx_t1_masks'][1].sum() == 0 and G['bx_t0_masks'][1].sum() > 0      # a scene without an object for one head
    assert G['az_t0_masks'].sum() == 0 and G['by_t1_masks'].sum() == 0           # num_pos == 0
    ai = G['ax_t0_inds'][0][G['ax_t0_masks'][0] == 1]
    assert (ai % W == 0).any() and (ai % W == W - 1).any() and (ai // W == 0).any() and (ai // W == H - 1).any()
    for c in 'ab':
        assert np.abs(G[c + '_p0_hm']).max() > 10


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run_targets(head, gt):
    ret = head.assign_targets(gt, feature_map_size=(H, W))
    return ret, [tuple(ret[k][h].cpu().numpy() for k in ('heatmaps', 'target_boxes', 'inds', 'masks')) for h in range(len(ret['heatmaps']))]


@gpu
def test_gpu_scatter_forward_backward():
    nx, ny, _ = (int(v) for v in G['sc_grid'])
    feats, coords = dev(G['sc_features']).requires_grad_(True), dev(G['sc_coords'])
    n, C = feats.shape
    grad = dev(G['sc_grad_out'])
    mod = PointPillarScatter(to_attr({'NUM_BEV_FEATURES': C}), (nx, ny, 1))
    out = mod({'pillar_features': feats, 'voxel_coords': coords, 'batch_size': B})['spatial_features']
    out.backward(grad)
    assert bits_equal(out.detach().cpu().numpy(), G['sc_out']) and bits_equal(feats.grad.cpu().numpy(), G['sc_grad_features'])
    # batch_size read from the coordinates when the key is absent
    out2 = mod({'pillar_features': feats.detach(), 'voxel_coords': coords})['spatial_features']
    assert bits_equal(out2.cpu().numpy(), G['sc_out'])
    # the padded form: 40 more rows of garbage behind the device count, plus skipped rows inside the count
    pad = 40
    fp = torch.cat([feats.detach(), torch.full((pad, C), 7.0, device='cuda')]).requires_grad_(True)
    cp = torch.cat([coords, coords[:pad]]).contiguous()
    count = torch.tensor([n], dtype=torch.int32, device='cuda')
    out3 = pillar_scatter(fp, cp, B, ny, nx, count=count)
    out3.backward(grad)
    assert bits_equal(out3.detach().cpu().numpy(), G['sc_out'])
    g3 = fp.grad.cpu().numpy()
    assert bits_equal(g3[:n], G['sc_grad_features']) and not g3[n:].any()
    bad = coords.clone()
    bad[0, 0], bad[1, 3], bad[2, 0] = B, nx * ny * 2, -1                        # batch index / cell outside: skipped
    f4 = feats.detach().clone().requires_grad_(True)
    out4 = pillar_scatter(f4, bad, B, ny, nx)
    out4.backward(grad)
    ref = G['sc_out'].copy().reshape(B, C, -1)
    for i in range(3):
        c = G['sc_coords'][i]
        ref[c[0], :, c[2] * nx + c[3]] = 0
    assert bits_equal(out4.detach().cpu().numpy().reshape(B, C, -1), ref)
    g4 = f4.grad.cpu().numpy()
    assert not g4[:3].any() and bits_equal(g4[3:], G['sc_grad_features'][3:])


@gpu
@pytest.mark.parametrize("c,t", BATCHES)
def test_gpu_targets(c, t):
    head = make_head(c).cuda()
    gt = dev(G[c + t + '_gt_boxes'])
    before = gt.clone()
    ret, got = run_targets(head, gt)
    off = check_targets(got, c, t)
    print("targets", c, t, "heat-map cells not bit-identical:", off)
    assert bits_equal(gt.cpu().numpy(), before.cpu().numpy()), "gt_boxes was written"
    _, again = run_targets(head, gt)
    for a, b in zip(got, again):
        for x, y in zip(a, b):
            assert bits_equal(x, y), "two runs differ"
    assert ret['heatmap_masks'] == []


def gpu_losses(head, c, t, targets=None):
    """The head's get_loss on the fixture's predictions -> (loss, tb_dict, leaves per head)."""
    if targets is None:
        targets = head.assign_targets(dev(G[c + t + '_gt_boxes']), feature_map_size=(H, W))
    leaves = [{k: dev(v).requires_grad_(True) for k, v in preds_of(c, h).items()} for h in range(n_heads(c))]
    head.forward_ret_dict = {'pred_dicts': [dict(d) for d in leaves], 'target_dicts': targets}
    loss, tb = head.get_loss()
    return loss, tb, leaves


@gpu
@pytest.mark.parametrize("c,t", BATCHES)
def test_gpu_losses(c, t):
    head = make_head(c).cuda()
    loss, tb, leaves = gpu_losses(head, c, t)
    loss.backward()
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 and v.is_cuda for v in tb.values())
    order = CONFIGS[c]['head']['SEPARATE_HEAD_CFG']['HEAD_ORDER']
    for h in range(n_heads(c)):
        grads = {k: leaves[h][k].grad.cpu().numpy() for k in ['hm'] + order}
        check_loss(c, t, h, float(tb['hm_loss_head_%d' % h]), float(tb['loc_loss_head_%d' % h]), grads)
    assert abs(float(loss.detach()) - float(G[c + t + '_loss'])) <= LOSS_TOL * 2 * n_heads(c)      # the sum of 2 * heads terms
    assert abs(float(tb['rpn_loss']) - float(loss.detach())) == 0


def focal_case(n):
    """Logits around -4 (a heat-map head past its -2.19 initialisation), a sparse heat map with values in [0, 0.95) and up to
    five cells that are exactly 1, the first and the last among them."""
    rng = np.random.default_rng(n)
    logits = rng.normal(-4.0, 1.0, n).astype(np.float32)
    hm = np.where(rng.random(n) < 0.05, rng.random(n) ** 2 * 0.95, 0.0).astype(np.float32)
    hm[np.unique(np.linspace(0, n - 1, min(n, 5)).astype(np.int64))] = 1.0
    return logits, hm


@gpu
@pytest.mark.parametrize("n,blocks", [(1, 1), (2049, 2), (2097153, 1024)])
def test_gpu_focal_loss_at_the_block_boundaries(n, blocks):
    """The sizes at which the shared partial sums (csrc/loss_sums.h) can go wrong: one element; one full workgroup of 2048
    and one element; one element past the 1024-workgroup cap, where the grid-stride loop wraps.  Against the float64
    restatement, within test_gpu_losses' bound."""
    assert _lib.load().pda_center_focal_blocks(n) == blocks
    logits, hm = focal_case(n)
    ref_loss, ref_grad = rs.focal_loss(logits, hm)
    x = dev(logits).requires_grad_(True)
    loss = cu.focal_loss(x, dev(hm))
    loss.backward()
    scale = float(np.abs(ref_grad).max())
    d_loss = abs(float(loss.detach()) - ref_loss)
    d_g = float(np.abs(x.grad.cpu().numpy().astype(np.float64) - ref_grad).max())
    print("focal n", n, "loss %.9g diff %.3g grad diff %.3g of %.3g" % (ref_loss, d_loss, d_g, scale))
    assert d_loss <= LOSS_TOL
    assert d_g <= LOSS_TOL * scale


@gpu
@pytest.mark.parametrize("c", "ab")
def test_gpu_decode_and_nms(c):
    cfg, pp = CONFIGS[c], CONFIGS[c]['head']['POST_PROCESSING']
    head = make_head(c).cuda().eval()
    pred_dicts = [{k: dev(v) for k, v in preds_of(c, h).items()} for h in range(n_heads(c))]
    p = c + 'x_'
    for h, names in enumerate(cfg['head']['CLASS_NAMES_EACH_HEAD']):
        pd = pred_dicts[h] if 'vel' in cfg['head']['SEPARATE_HEAD_CFG']['HEAD_ORDER'] else {k: v for k, v in pred_dicts[h].items() if k != 'vel'}
        boxes, scores, labels = cu.decode_topk(pd, pp['MAX_OBJ_PER_SAMPLE'], head.class_id_mapping_each_head[h], head.point_cloud_range,
                                               head.voxel_size, head.feature_map_stride, pp['POST_CENTER_LIMIT_RANGE'], pp['SCORE_THRESH'])
        _, ind = torch.topk(pd['hm'].reshape(B, -1), boxes.shape[1])
        check_decode(c, h, ind.cpu().numpy(), boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy())
        selected, _, num = model_nms_utils.class_agnostic_nms_batched(scores, boxes, pp['NMS_CONFIG'], valid=scores > float('-inf'))
        for s in range(B):
            rows = np.nonzero(scores[s].cpu().numpy() > -np.inf)[0]
            ref_keep = rows[G['%sd%d_s%d_keep' % (p, h, s)]]
            assert int(num[s]) == len(ref_keep) and np.array_equal(selected[s, :len(ref_keep)].cpu().numpy(), ref_keep), "keep list"
            assert (selected[s, len(ref_keep):] == -1).all()
    padded = head.generate_predicted_boxes(B, pred_dicts)
    counts = padded['num_pred'].tolist()
    for s in range(B):
        rb, rsc, rl = (G['%sf_s%d_%s' % (p, s, k)] for k in ('pred_boxes', 'pred_scores', 'pred_labels'))
        n = counts[s]
        assert n == len(rb) and n > 0
        b = padded['pred_boxes'][s].cpu().numpy()
        assert np.array_equal(padded['pred_labels'][s, :n].cpu().numpy(), rl) and not padded['pred_labels'][s, n:].any()
        assert bits_equal(b[:n, 2], rb[:, 2]) and bits_equal(b[:n, 7:], rb[:, 7:]) and not b[n:].any()
        assert ulps(b[:n, [0, 1, 3, 4, 5, 6]], rb[:, [0, 1, 3, 4, 5, 6]]).max() <= 2
        assert ulps(padded['pred_scores'][s, :n].cpu().numpy(), rsc).max() <= 2 and not padded['pred_scores'][s, n:].any()
    # the padded form feeds the recall counters and to_pred_dicts unchanged
    gt_np = np.nan_to_num(G[p + 'gt_boxes'], nan=0.5)           # recall_record is not specified for NaN columns
    gt = dev(gt_np)
    rec = model_nms_utils.recall_record(padded['pred_boxes'], padded['num_pred'], gt, [0.3, 0.5, 0.7])
    assert rec.shape == (4,) and int(rec[0]) == kept_gt(gt_np)
    dicts = model_nms_utils.to_pred_dicts(padded)
    assert [len(d['pred_boxes']) for d in dicts] == counts and dicts[0]['pred_labels'].min() >= 1
    rois, roi_scores, roi_labels = head.reorder_rois_for_refining(B, padded)
    assert rois.shape[:2] == roi_scores.shape == roi_labels.shape and roi_labels.dtype == torch.int64
    head.predict_boxes_when_training = True
    out = head.train()({'spatial_features_2d': torch.zeros(B, 16, H, W, device='cuda'), 'gt_boxes': gt, 'batch_size': B})
    assert out['has_class_labels'] is True and out['rois'].shape[0] == B and out['roi_labels'].shape == out['roi_scores'].shape


@gpu
def test_gpu_graph_replay_equals_eager():
    """assign_targets + get_loss + backward from one captured graph, bit for bit the eager run -- apart from the regression
    gradient at the cell three objects share, where the order of the float atomicAdd may differ: within 1 ulp there."""
    c, t = 'b', 'x'
    head = make_head(c).cuda()
    gt = dev(G[c + t + '_gt_boxes'])
    order = ['hm'] + CONFIGS[c]['head']['SEPARATE_HEAD_CFG']['HEAD_ORDER']
    leaves = [{k: dev(v).requires_grad_(True) for k, v in preds_of(c, h).items()} for h in range(n_heads(c))]
    flat = [d[k] for d in leaves for k in order]

    def step():
        targets = head.assign_targets(gt, feature_map_size=(H, W))
        head.forward_ret_dict = {'pred_dicts': [dict(d) for d in leaves], 'target_dicts': targets}
        loss, tb = head.get_loss()
        return loss, torch.autograd.grad(loss, flat), targets

    loss_e, grads_e, targets_e = step()
    eager = [loss_e.detach().clone()] + [g.clone() for g in grads_e] + [x.clone() for x in targets_e['heatmaps'] + targets_e['target_boxes']]
    del loss_e, grads_e, targets_e
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g, grads_g, targets_g = step()
    graph.replay()
    torch.cuda.synchronize()
    replay = [loss_g.detach()] + list(grads_g) + targets_g['heatmaps'] + targets_g['target_boxes']
    cell = 25 * W + 25
    n_flat = 1 + len(flat)
    for i, (a, b) in enumerate(zip(eager, replay)):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        head_idx, name = divmod(i - 1, len(order)) if 1 <= i < n_flat else (None, None)
        if head_idx == 1 and order[name] != 'hm':
            a, b = a.reshape(B, a.shape[1], -1).copy(), b.reshape(B, b.shape[1], -1).copy()
            assert ulps(a[0, :, cell], b[0, :, cell]).max() <= 1
            a[0, :, cell] = b[0, :, cell] = 0
        assert bits_equal(a, b), "replay differs from the eager run at output %d" % i


@gpu
def test_gpu_centerpoint_train_and_eval():
    from pdanet_amd import synth
    torch.manual_seed(3)
    model = CenterPoint(to_attr(centerpoint_cfg()), 3, DATASET).cuda()
    pts = synth.batch_points(B, 2048)
    pts[:, 1:4] *= 0.1                                        # the ONCE range of synth.py into this 15 m x 13 m range
    batch = {'points': dev(pts), 'gt_boxes': dev(G['ax_gt_boxes']), 'batch_size': B}
    model.train()
    ret, tb, disp = model(dict(batch))
    assert torch.isfinite(ret['loss']) and disp == {} and set(tb) == {'loss_rpn', 'hm_loss_head_0', 'loc_loss_head_0', 'rpn_loss'}
    ret['loss'].backward()
    for name, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    model.eval()
    with torch.no_grad():
        pred_dicts, recall = model(dict(batch))
    assert len(pred_dicts) == B and set(pred_dicts[0]) == {'pred_boxes', 'pred_scores', 'pred_labels'}
    assert recall['gt'] == kept_gt(G['ax_gt_boxes']) and 'rcnn_0.5' in recall
