"""SECOND-IoU: the rotated BEV RoI-grid pool (csrc/bev_roi_pool.hip), the points-per-box count (csrc/roi_pool.hip), SECONDHead
and SECONDNetIoU against the reference's own CPU run (tests/golden/second_iou.npz, made by make_second_iou_golden.py) and a
float64 numpy restatement of the pooling (tests/golden/bev_roi_pool_restatement.py).

Tolerances.  The pooling on the lattice is exact in float32 whatever the order, so the device must give the fixture's bits.
In general position the bound is computed here, never from the kernel: 4 x the largest error of torch's own float32 CPU
composition against the float64 restatement on the same inputs, plus 2^-23 x max |out| -- both are float32 evaluations of
one formula that differ only in operation order and contraction.  The head follows test_voxel_rcnn.py: the fixture is the
reference's float32 CPU run, its error against a float64 run of the same head is measured here, and the device may be off by
FACTOR times that; a scalar loss gets 2^-23 on top, because a float32 scalar lands closer than an ulp to the float64 value
only by luck.  Every figure is printed."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from pdanet_amd.config import to_attr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import bev_roi_pool_restatement as rs  # noqa: E402

gpu = pytest.mark.gpu
FACTOR = 4.0
EPS32 = 2.0 ** -23
with open(os.path.join(HERE, "golden", "second_iou_state_dict.json")) as _f:
    FIXTURE = json.load(_f)
CFG = FIXTURE['config']
# geometry of the fixture's pooling cases: (G, min_x, min_y, cell)
LAT = dict(G=4, min_x=0.0, min_y=0.0, cell=0.125 * 8)
GEN = dict(G=7, min_x=0.0, min_y=-5.0, cell=0.05 * 8)
HEAD_PCR, HEAD_VOXEL = [0.0, -2.4, -3.0, 4.0, 2.4, 1.0], [0.05, 0.05, 0.1]
LOSSES = ('BinaryCrossEntropy', 'L2', 'smoothL1')
VARIANTS = ('default', 'iou', 'cls', 'weighted_iou_cls', 'num_pts_iou_cls', 'score_by_class')


@pytest.fixture(scope="module")
def npz():
    with np.load(os.path.join(HERE, "golden", "second_iou.npz")) as f:
        return {k: f[k] for k in f.files}


def restate(bev, rois, geo, dtype=np.float64):
    return rs.roi_grid_pool(bev, rois, geo['G'], geo['min_x'], geo['min_y'], geo['cell'], geo['cell'], dtype)


def composed_cpu(bev, rois, geo):
    """torch's own float32 composition on the CPU"""
    from pdanet_amd.second_head import bev_roi_grid_pool_composed
    return bev_roi_grid_pool_composed(torch.from_numpy(bev), torch.from_numpy(rois), geo['G'], geo['min_x'], geo['min_y'],
                                      geo['cell'], geo['cell']).numpy()


def fused_gpu(bev, rois, geo):
    from pdanet_amd.second_head import bev_roi_grid_pool
    return bev_roi_grid_pool(torch.from_numpy(bev).cuda(), torch.from_numpy(rois).cuda(), geo['G'], geo['min_x'], geo['min_y'],
                             geo['cell'], geo['cell'])


@pytest.fixture(scope="module")
def general(npz):
    """The two general-position runs (C = 6 from the fixture, C = 130 drawn here), each with its float64 truth and its bound,
    computed once."""
    rng = np.random.default_rng(130)
    cases = {6: npz["gen_bev"], 130: rng.standard_normal((2, 130, 25, 22)).astype(np.float32)}
    out = {}
    for c, bev in cases.items():
        truth = restate(bev, npz["gen_rois"], GEN)
        e_torch = float(np.abs(composed_cpu(bev, npz["gen_rois"], GEN) - truth).max())
        out[c] = dict(bev=bev, truth=truth, e_torch=e_torch, bound=FACTOR * e_torch + EPS32 * float(np.abs(truth).max()))
    return out


# ---- without a GPU --------------------------------------------------------------------------------------------------------
def test_state_dict_layout_is_the_references():
    from pdanet_amd.second_head import SECONDHead
    from pdanet_amd.second_net_iou import SECONDNetIoU
    roi_cfg = CFG['MODEL']['ROI_HEAD']
    before = json.dumps(CFG['MODEL'], sort_keys=True)
    head = SECONDHead(backbone_channels={}, model_cfg=to_attr(roi_cfg), point_cloud_range=CFG['dataset']['point_cloud_range'],
                      voxel_size=CFG['dataset']['voxel_size'], num_class=1)
    assert [[k, list(v.shape)] for k, v in head.state_dict().items()] == FIXTURE['SECONDHead']
    # the Dropout sits between the two shared blocks and after the first iou block, as in the reference
    assert [type(m).__name__ for m in head.shared_fc_layer] == ['Conv1d', 'BatchNorm1d', 'ReLU', 'Dropout', 'Conv1d', 'BatchNorm1d', 'ReLU']
    assert [type(m).__name__ for m in head.iou_layers] == ['Conv1d', 'BatchNorm1d', 'ReLU', 'Dropout', 'Conv1d', 'BatchNorm1d', 'ReLU', 'Conv1d']
    assert (head.cell_x, head.cell_y) == (0.05 * 8, 0.05 * 8) and (head.min_x, head.min_y) == (0.0, -0.4)
    model = SECONDNetIoU(to_attr(CFG['MODEL']), 3, CFG['dataset'])
    own = model.state_dict()
    assert [[k, list(v.shape)] for k, v in own.items()] == FIXTURE['SECONDNetIoU']
    assert [n for n, _ in model.named_children()] == ['vfe', 'backbone_3d', 'map_to_bev_module', 'backbone_2d', 'dense_head', 'roi_head']
    assert json.dumps(CFG['MODEL'], sort_keys=True) == before                      # the config is not modified
    sd = {k: torch.zeros(shape, dtype=own[k].dtype) for k, shape in FIXTURE['SECONDNetIoU']}
    SECONDNetIoU(to_attr(CFG['MODEL']), 3, CFG['dataset']).load_state_dict(sd, strict=True)


def test_refusals():
    from pdanet_amd import model_nms_utils
    from pdanet_amd.second_head import SECONDHead
    from pdanet_amd.second_net import SECONDNet
    from pdanet_amd.second_net_iou import SECONDNetIoU
    ds = CFG['dataset']
    cfg = json.loads(json.dumps(CFG['MODEL']))
    cfg['ROI_HEAD']['LOSS_CONFIG']['IOU_LOSS'] = 'focalbce'
    with pytest.raises(NotImplementedError, match="focalbce"):
        SECONDHead(backbone_channels={}, model_cfg=to_attr(cfg['ROI_HEAD']), point_cloud_range=ds['point_cloud_range'],
                   voxel_size=ds['voxel_size'], num_class=1)
    with pytest.raises(NotImplementedError, match="focalbce"):
        SECONDNetIoU(to_attr(cfg), 3, ds)
    cfg = json.loads(json.dumps(CFG['MODEL']))
    cfg['POST_PROCESSING']['NMS_CONFIG']['MULTI_CLASSES_NMS'] = True
    with pytest.raises(NotImplementedError, match="MULTI_CLASSES_NMS"):
        SECONDNetIoU(to_attr(cfg), 3, ds)
    with pytest.raises(NotImplementedError, match="MULTI_CLASSES_NMS"):
        model_nms_utils.post_processing_iou({}, to_attr(cfg['POST_PROCESSING']), 3, ds['class_names'])
    cfg['POST_PROCESSING']['NMS_CONFIG']['MULTI_CLASSES_NMS'] = False
    cfg['POST_PROCESSING']['OUTPUT_RAW_SCORE'] = True
    with pytest.raises(NotImplementedError, match="OUTPUT_RAW_SCORE"):
        model_nms_utils.post_processing_iou({}, to_attr(cfg['POST_PROCESSING']), 3, ds['class_names'])
    cfg = json.loads(json.dumps(CFG['MODEL']))
    del cfg['ROI_HEAD']
    with pytest.raises(ValueError, match="ROI_HEAD"):
        SECONDNetIoU(to_attr(cfg), 3, ds)
    for other in ('VoxelRCNNHead', 'PartA2FCHead'):
        cfg = json.loads(json.dumps(CFG['MODEL']))
        cfg['ROI_HEAD']['NAME'] = other
        with pytest.raises(NotImplementedError, match=other):
            SECONDNetIoU(to_attr(cfg), 3, ds)
    with pytest.raises(NotImplementedError):                                       # SECONDNet still has no RoI head
        SECONDNet(to_attr(CFG['MODEL']), 3, ds)


def test_symbols_exist_and_sizes_are_checked_before_any_launch():
    from pdanet_amd import build, _lib
    build.build()
    lib = _lib.load()
    for name in ("pda_bev_roi_grid_pool", "pda_points_in_boxes_count"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    f = ctypes.c_float
    pool = lambda b, r, c, h, w, g: lib.pda_bev_roi_grid_pool(None, None, None, b, r, c, h, w, g, f(0), f(0), f(0.4), f(0.4), None)
    assert pool(0, 128, 512, 200, 176, 7) == 0 and pool(4, 0, 512, 200, 176, 7) == 0          # empty: returns at once
    for bad, word in (((2, 8, 5, 1, 9, 4), b"h - 1"), ((2, 8, 5, 17, 1, 4), b"w - 1"), ((2, 8, 5, 17, 9, 0), b"grid"),
                      ((2, 8, 5, 17, 9, 17), b"grid"), ((2, 8, 0, 17, 9, 4), b"channels"), ((2, 4097, 5, 17, 9, 4), b"rois"),
                      ((65536, 8, 5, 17, 9, 4), b"batch"), ((-1, 8, 5, 17, 9, 4), b"batch")):
        assert pool(*bad) == 1 and word in lib.pda_last_error(), bad
    assert pool(2, 8, 5, 17, 9, 4) == 1 and b"null" in lib.pda_last_error()
    assert lib.pda_points_in_boxes_count(None, 5, None, None, 100, 0, 5, None) == 0
    assert lib.pda_points_in_boxes_count(None, 3, None, None, 100, 2, 5, None) == 1 and b"stride" in lib.pda_last_error()
    assert lib.pda_points_in_boxes_count(None, 5, None, None, 100, 2, 5, None) == 1 and b"null" in lib.pda_last_error()


def lattice_kinds(npz):
    return rs.classify(npz["lat_rois"], LAT['G'], 17, 9, LAT['min_x'], LAT['min_y'], LAT['cell'], LAT['cell']).reshape(-1)


def test_restatement_reproduces_the_reference_run(npz, general):
    """The fixture is the reference's own float32 run: bit for bit on the lattice, to float32 accuracy in general position.
    The lattice RoIs cover what they were built to cover; this is asserted on the golden values alone."""
    lat = restate(npz["lat_bev"], npz["lat_rois"], LAT)
    assert npz["lat_out"].dtype == np.float32 and npz["lat_out"].shape == (32, 5, 4, 4)
    assert np.array_equal(npz["lat_out"].astype(np.float64), lat)
    assert np.array_equal(restate(npz["lat_bev"], npz["lat_rois"], LAT, np.float32), npz["lat_out"])     # exact in float32 too
    rois = npz["lat_rois"].reshape(-1, 7)
    assert np.all(rois[:, :2] * 8 == np.round(rois[:, :2] * 8)) and np.all(rois[:, 3:6] * 2 == np.round(rois[:, 3:6] * 2))
    assert np.all(rois[:, 6] == 0) and int((np.abs(rois).sum(1) == 0).sum()) == 1 and np.all(np.abs(npz["lat_bev"]) <= 8)
    assert np.array_equal(npz["lat_bev"], np.round(npz["lat_bev"]))
    kinds = lattice_kinds(npz)
    print("lattice RoIs:", {k: int((kinds == k).sum()) for k in sorted(set(kinds))})
    assert (kinds == 'inside').sum() * 4 >= len(kinds)
    cut = [k for k in kinds if k not in ('inside', 'outside')]
    assert len(cut) >= 8 and all(any(side in k for k in cut) for side in 'lrtb')
    outside = kinds == 'outside'
    assert outside.sum() >= 4 and not npz["lat_out"][outside].any() and npz["lat_out"][~outside].any(axis=(1, 2, 3)).sum() >= 24
    e = float(np.abs(npz["gen_out"] - general[6]['truth']).max())
    print("general case: reference in float32 against the float64 restatement %.3e, this torch on the CPU %.3e, max |out| %.3f"
          % (e, general[6]['e_torch'], float(np.abs(general[6]['truth']).max())))
    # positions up to 25 cells carry a few float32 roundings (~1e-5 of a cell), features change by a few units per cell
    assert e < 2e-4 and general[6]['e_torch'] < 2e-4 and general[130]['e_torch'] < 2e-4
    assert np.abs(npz["gen_rois"][..., 6]).max() > 3 and npz["gen_out"].shape == (24, 6, 7, 7)


def make_head(npz, loss='BinaryCrossEntropy'):
    from pdanet_amd.second_head import SECONDHead
    cfg = json.loads(str(npz["head_cfg"]))
    cfg['LOSS_CONFIG']['IOU_LOSS'] = loss
    head = SECONDHead(backbone_channels={}, model_cfg=to_attr(cfg), point_cloud_range=HEAD_PCR, voxel_size=HEAD_VOXEL, num_class=1)
    head.load_state_dict({k[len("head_sd."):]: torch.from_numpy(v) for k, v in npz.items() if k.startswith("head_sd.")}, strict=True)
    return head


def head_batch(npz, device, dtype=torch.float32):
    rois = torch.from_numpy(npz["head_rois"]).to(device=device, dtype=dtype)
    return {'batch_size': 2, 'rois': rois, 'roi_scores': torch.zeros(rois.shape[:2], device=device),
            'roi_labels': torch.ones(rois.shape[:2], dtype=torch.long, device=device),
            'spatial_features_2d': torch.from_numpy(npz["head_bev"]).to(device=device, dtype=dtype)}


def head_run(npz, device, dtype=torch.float32, pool=None):
    """eval rcnn_iou (before the step), then one train forward: rcnn_iou, the three losses with every parameter's gradient,
    the running statistics after it -- the generator's sequence.  pool: a replacement for roi_grid_pool."""
    head = make_head(npz).to(device=device, dtype=dtype)
    if pool is not None:
        head.roi_grid_pool = pool
    res = {}
    head.eval()
    with torch.no_grad():
        bd = head(head_batch(npz, device, dtype))
        assert bd['batch_box_preds'] is bd['rois'] and bd['cls_preds_normalized'] is False
        res['rcnn_iou_eval'] = bd['batch_cls_preds'].cpu().numpy()
    head.train()
    pooled = head.roi_grid_pool(head_batch(npz, device, dtype))
    assert not pooled.requires_grad
    rcnn_iou = head.iou_layers(head.shared_fc_layer(pooled.view(pooled.shape[0], -1, 1))).transpose(1, 2).contiguous().squeeze(dim=1)
    res['pooled'], res['rcnn_iou_train'] = pooled.cpu().numpy(), rcnn_iou.detach().cpu().numpy()
    labels = torch.from_numpy(npz["head_labels"]).to(device=device, dtype=dtype)
    names, params = zip(*head.named_parameters())
    for loss_name in LOSSES:
        head.model_cfg['LOSS_CONFIG']['IOU_LOSS'] = loss_name
        loss, tb = head.get_box_iou_layer_loss({'rcnn_iou': rcnn_iou, 'rcnn_cls_labels': labels})
        assert set(tb) == {'rcnn_loss_iou'} and tb['rcnn_loss_iou'].dim() == 0 and tb['rcnn_loss_iou'].device.type == device
        grads = torch.autograd.grad(loss, params, retain_graph=True)
        res['loss.' + loss_name] = float(loss.detach())
        res['grad.' + loss_name] = {n: g.cpu().numpy() for n, g in zip(names, grads)}
    res['stats'] = {k: v.detach().cpu().numpy() for k, v in head.named_buffers() if 'running' in k}
    assert all(int(v) == 1 for k, v in head.named_buffers() if k.endswith('num_batches_tracked'))
    return res


def golden_head(npz):
    res = {'rcnn_iou_eval': npz["head_rcnn_iou_eval"], 'rcnn_iou_train': npz["head_rcnn_iou_train"], 'pooled': npz["head_pooled"]}
    for loss_name in LOSSES:
        res['loss.' + loss_name] = float(npz["head_loss." + loss_name])
        pre = "head_grad.%s." % loss_name
        res['grad.' + loss_name] = {k[len(pre):]: v for k, v in npz.items() if k.startswith(pre)}
    res['stats'] = {k[len("head_after."):]: v for k, v in npz.items() if k.startswith("head_after.") and 'running' in k}
    return res


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def together(got, ref):
    """one figure over a dict of tensors, normalised by the largest reference entry"""
    assert set(got) == set(ref)
    scale = max(float(np.abs(np.asarray(r, np.float64)).max()) for r in ref.values())
    return max(float(np.abs(np.asarray(got[k], np.float64) - np.asarray(ref[k], np.float64)).max()) for k in ref) / scale


def head_figures(got, truth):
    fig = {k: rel(got[k], truth[k]) for k in ('rcnn_iou_eval', 'rcnn_iou_train', 'pooled')}
    for loss_name in LOSSES:
        fig['loss.' + loss_name] = abs(got['loss.' + loss_name] - truth['loss.' + loss_name]) / abs(truth['loss.' + loss_name])
        fig['grad.' + loss_name] = together(got['grad.' + loss_name], truth['grad.' + loss_name])
    fig['stats'] = together(got['stats'], truth['stats'])
    return fig


@pytest.fixture(scope="module")
def head_truth(npz):
    """The head in float64 on the CPU over the float64 restatement of the pooling, once, and the fixture's error against it."""
    def pool(bd):
        geo = dict(G=4, min_x=HEAD_PCR[0], min_y=HEAD_PCR[1], cell=HEAD_VOXEL[0] * 8)
        return torch.from_numpy(restate(bd['spatial_features_2d'].numpy(), bd['rois'].numpy(), geo))
    truth = head_run(npz, "cpu", torch.float64, pool)
    return truth, head_figures(golden_head(npz), truth)


def test_head_losses_and_gradients_on_the_cpu(npz, head_truth, monkeypatch):
    """CPU tensors take the composed pooling; the same arithmetic as the reference's run, so the figures are rounding only."""
    from pdanet_amd import second_head
    monkeypatch.setenv(second_head.ENV, "composed")
    truth, e_gold = head_truth
    got = head_run(npz, "cpu")
    gold = golden_head(npz)
    assert len(gold['grad.L2']) == 14 and len(gold['stats']) == 8
    for k, e in head_figures(got, gold).items():
        print("head on the CPU against the reference run, %s: %.3e (reference against float64: %.3e)" % (k, e, e_gold[k]))
        assert e <= 1e-5, k
    for k, e in e_gold.items():
        assert e < 2e-4, k
    monkeypatch.setenv(second_head.ENV, "neither")
    with pytest.raises(ValueError):
        make_head(npz).roi_grid_pool(head_batch(npz, "cpu"))


def test_score_rules_on_the_cpu(npz):
    """The two score rules that need no kernel, against the values the reference's post_processing handed to its NMS."""
    from pdanet_amd import model_nms_utils as mu
    iou = torch.sigmoid(torch.from_numpy(npz["post_iou_logits"])).max(dim=-1)[0]
    cls = torch.sigmoid(torch.from_numpy(npz["post_cls_logits"]))
    labels = torch.from_numpy(npz["post_labels"])
    assert sorted(set(labels[1].tolist())) == [1, 3]
    cfg = json.loads(str(npz["post.score_by_class.cfg"]))['NMS_CONFIG']
    got = mu.nms_scores_by_class(iou, cls, labels, cfg['SCORE_BY_CLASS'], [str(n) for n in npz["post_class_names"]])
    assert np.allclose(got.numpy(), npz["post.score_by_class.nms_scores"], rtol=0, atol=1e-6)
    assert not got[1][labels[1] == 3].any() and got[0][labels[0] == 3].any()       # scene 1: two distinct labels, class 3 unscored
    cfg = json.loads(str(npz["post.num_pts_iou_cls.cfg"]))['NMS_CONFIG']
    counts = torch.from_numpy(npz["post_point_counts"])
    got = mu.scores_by_npoints(cls, iou, counts, cfg['SCORE_THRESH']['cls'], cfg['SCORE_THRESH']['iou'])
    assert np.allclose(got.numpy(), npz["post.num_pts_iou_cls.nms_scores"], rtol=0, atol=1e-6)
    n = npz["post_point_counts"]
    assert (n <= 10).any() and (n >= 40).any() and ((n > 10) & (n < 40)).any()
    with pytest.raises(NotImplementedError):
        mu.nms_scores_by_class(iou, cls, labels, {'Car': 'iou', 'Pedestrian': 'weighted', 'Cyclist': 'iou'}, ['Car', 'Pedestrian', 'Cyclist'])


# ---- on the GPU -----------------------------------------------------------------------------------------------------------
@gpu
def test_gpu_lattice_case_is_bitwise(npz):
    out = fused_gpu(npz["lat_bev"], npz["lat_rois"], LAT)
    assert out.shape == (32, 5, 4, 4) and out.dtype == torch.float32 and not out.requires_grad
    assert torch.equal(out.cpu(), torch.from_numpy(npz["lat_out"]))


@gpu
@pytest.mark.parametrize("channels", [6, 130])
def test_gpu_general_case(npz, general, channels):
    case = general[channels]
    out = fused_gpu(case['bev'], npz["gen_rois"], GEN).cpu().numpy()
    err = float(np.abs(out - case['truth']).max())
    print("general case, C = %d: device %.3e, torch in float32 on the CPU %.3e, bound %.3e, max |out| %.3f"
          % (channels, err, case['e_torch'], case['bound'], float(np.abs(case['truth']).max())))
    assert out.shape == (24, channels, 7, 7)
    assert err <= case['bound']


@gpu
def test_gpu_hostile_rois(npz):
    """NaN, +inf and 1e30 boxes read nothing and give zeros; every other row keeps its bits.  (The position-to-corners
    function ran under the host sanitizers first: tools/bev_roi_grid_check.cpp.)"""
    rois = npz["lat_rois"].copy()
    kinds = lattice_kinds(npz).reshape(2, 16)
    rows = [(0, int(np.flatnonzero(kinds[0] == 'inside')[0])), (1, int(np.flatnonzero(kinds[1] == 'inside')[0])),
            (1, int(np.flatnonzero(kinds[1] == 'inside')[1]))]
    for (b, r), value in zip(rows, (np.nan, np.inf, 1e30)):
        rois[b, r] = value
    out = fused_gpu(npz["lat_bev"], rois, LAT).cpu().numpy()
    want = npz["lat_out"].copy()
    for b, r in rows:
        assert want[b * 16 + r].any()
        want[b * 16 + r] = 0
    assert np.array_equal(out, want)
    # one hostile field is enough, wherever it sits
    for col in (0, 1, 3, 4, 6):
        rois = npz["lat_rois"].copy()
        rois[0, rows[0][1], col] = np.nan
        out = fused_gpu(npz["lat_bev"], rois, LAT).cpu().numpy()
        assert not out[rows[0][1]].any() and np.array_equal(np.delete(out, rows[0][1], 0), np.delete(npz["lat_out"], rows[0][1], 0))


@gpu
def test_gpu_fused_equals_composed(npz, general, monkeypatch):
    from pdanet_amd import second_head
    head = make_head(npz)
    head.min_x, head.min_y, head.cell_x, head.cell_y, head.pool_cfg = GEN['min_x'], GEN['min_y'], GEN['cell'], GEN['cell'], {'GRID_SIZE': 7}
    res = {}
    for path in ("fused", "composed"):
        monkeypatch.setenv(second_head.ENV, path)
        bd = {'rois': torch.from_numpy(npz["gen_rois"]).cuda(), 'spatial_features_2d': torch.from_numpy(general[6]['bev']).cuda()}
        res[path] = head.roi_grid_pool(bd).cpu().numpy()
    err = float(np.abs(res["fused"] - res["composed"]).max())
    e_comp = float(np.abs(res["composed"] - general[6]['truth']).max())
    print("fused against composed on the device: %.3e (composed against float64 %.3e), bound %.3e" % (err, e_comp, general[6]['bound']))
    assert err <= general[6]['bound']


def _count_case():
    """Two scenes of 300 and 513 points with 1 + 3 + 2 columns in a shuffled order, five boxes each (the last the zero box),
    and one point with batch value 7.  Every point is at least 0.05 away from every face of every box of its scene (the
    faces of the test: dx/2 + 0.01 and dy/2 + 0.01 in the box frame, dz/2), so float32 and float64 agree on every decision."""
    rng = np.random.default_rng(55)
    boxes = np.zeros((2, 5, 7), np.float32)
    for b in range(2):
        boxes[b, :4, 0:2] = rng.uniform(-6, 6, (4, 2))
        boxes[b, :4, 2] = rng.uniform(-1, 0, 4)
        boxes[b, :4, 3:6] = rng.uniform([2.0, 1.2, 1.4], [5.0, 3.0, 2.2], (4, 3))
        boxes[b, :4, 6] = rng.uniform(-3.1, 3.1, 4)
    rows, want = [], np.zeros((2, 5), np.int64)
    for b, n in enumerate((300, 513)):
        kept = np.zeros((0, 3))
        while len(kept) < n:
            # half of the draws anywhere in the scene, half around the centres of the boxes
            near = boxes[b, rng.integers(0, 4, 2 * n), :3] + rng.normal(0, 1.2, (2 * n, 3))
            p = np.concatenate([rng.uniform([-9, -9, -2.5], [9, 9, 1.5], (2 * n, 3)), near])[rng.permutation(4 * n)]
            p = p.astype(np.float32).astype(np.float64)
            clear = np.ones(len(p), bool)
            for k in range(5):
                cx, cy, cz, dx, dy, dz, rz = boxes[b, k].astype(np.float64)
                sx, sy = p[:, 0] - cx, p[:, 1] - cy
                lx, ly = sx * np.cos(-rz) - sy * np.sin(-rz), sx * np.sin(-rz) + sy * np.cos(-rz)
                for d, half in ((np.abs(lx), dx / 2 + 0.01), (np.abs(ly), dy / 2 + 0.01), (np.abs(p[:, 2] - cz), dz / 2)):
                    clear &= np.abs(d - half) > 0.05
            kept = np.concatenate([kept, p[clear]])[:n]
        for k in range(5):
            cx, cy, cz, dx, dy, dz, rz = boxes[b, k].astype(np.float64)
            sx, sy = kept[:, 0] - cx, kept[:, 1] - cy
            lx, ly = sx * np.cos(-rz) - sy * np.sin(-rz), sx * np.sin(-rz) + sy * np.cos(-rz)
            want[b, k] = int(((np.abs(kept[:, 2] - cz) <= dz / 2) & (np.abs(lx) < dx / 2 + 0.01) & (np.abs(ly) < dy / 2 + 0.01)).sum())
        rows.append(np.concatenate([np.full((n, 1), b), kept, rng.random((n, 2))], axis=1))
    stray = np.concatenate([[7.0], boxes[0, 0, :3], [0.5, 0.5]])[None]              # the centre of a box, in no scene
    points = np.concatenate(rows + [stray]).astype(np.float32)
    return points[rng.permutation(len(points))], boxes, want


@gpu
def test_gpu_point_counts():
    from pdanet_amd.roiaware_pool3d_utils import points_in_boxes_count, points_in_boxes_cpu
    points, boxes, want = _count_case()
    assert points.shape == (814, 6) and want[:, :4].min() > 0 and not want[:, 4].any()
    p, b = torch.from_numpy(points).cuda(), torch.from_numpy(boxes).cuda()
    counts = points_in_boxes_count(p, b)
    assert counts.shape == (2, 5) and counts.dtype == torch.int32
    for s in range(2):
        mask = points_in_boxes_cpu(p[p[:, 0] == s][:, 1:4].contiguous(), b[s])
        assert torch.equal(counts[s].long(), mask.sum(dim=1).long())
    print("points per box:", counts.tolist())
    assert np.array_equal(counts.cpu().numpy(), want)
    assert torch.equal(points_in_boxes_count(p[:0], b), torch.zeros_like(counts))


# The running statistics are left by torch's own Conv1d and BatchNorm launches, not by this project's arithmetic, and the CPU
# run accumulates them in float64, so the 4x rule does not bind them (as in test_voxel_rcnn.py).  A float32 sum of n terms in
# any order is within (n - 1) 2^-24 of the exact sum relative to the sum of magnitudes: the widest dot product in front of a
# BatchNorm here has 128 terms (8 channels x 4 x 4), a batch mean and a batch variance are two sums over the 16 RoIs, and the
# momentum update adds three roundings.
TORCH_STATS_BOUND = (128 + 2 * 16 + 3) * 2.0 ** -24


@gpu
def test_gpu_head_against_the_reference(npz, head_truth, monkeypatch):
    from pdanet_amd import second_head
    monkeypatch.setenv(second_head.ENV, "fused")
    truth, e_gold = head_truth
    fig = head_figures(head_run(npz, "cuda"), truth)
    failed = []
    for k, e in fig.items():
        bound = FACTOR * e_gold[k] + (EPS32 if k.startswith('loss.') else 0.0)
        if k == 'stats':
            bound = max(bound, TORCH_STATS_BOUND)
        print("head %s: device %.3e, reference in float32 on the CPU %.3e, bound %.3e" % (k, e, e_gold[k], bound))
        if e > bound:
            failed.append(k)
    assert not failed, failed


@gpu
def test_gpu_head_training_path_reads_nothing(npz):
    """forward (proposal_layer, assign_targets, pooling, fc stacks) + loss + backward under sync debug mode 2."""
    gt = np.zeros((2, 3, 8), np.float32)
    gt[0, 0], gt[0, 1], gt[1, 0] = npz["head_rois"][0, 0].tolist() + [1], npz["head_rois"][0, 3].tolist() + [1], npz["head_rois"][1, 1].tolist() + [1]
    gt[..., :3] += 0.05

    batches = {seed: dict(head_batch(npz, "cuda"), gt_boxes=torch.from_numpy(gt).cuda(), roi_target_seed=seed) for seed in (1, 2)}

    def step(head, seed):
        head(batches[seed])                              # the uploads above are not part of the training path
        loss, tb = head.get_loss()
        loss.backward()
        return loss, tb

    head = make_head(npz).cuda().train()
    step(head, 1)                                        # loads the library and warms every lazy initialisation
    head.zero_grad()
    torch.cuda.set_sync_debug_mode(2)                    # a synchronising call raises
    try:
        loss, tb = step(head, 2)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert set(tb) == {'rcnn_loss_iou', 'rcnn_loss'} and all(v.dim() == 0 and v.is_cuda for v in tb.values())
    assert torch.isfinite(loss) and head.forward_ret_dict['rcnn_iou'].shape == (2 * 128, 1)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in head.parameters())


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_gpu_post_processing(npz, variant):
    from pdanet_amd import model_nms_utils as mu
    cfg = to_attr(json.loads(str(npz["post.%s.cfg" % variant])))
    assert ('SCORE_TYPE' in cfg['NMS_CONFIG']) == (variant != 'default')
    t = lambda k: torch.from_numpy(npz[k]).cuda()
    bd = {'batch_size': 2, 'batch_box_preds': t("post_rois"), 'batch_cls_preds': t("post_iou_logits"), 'roi_scores': t("post_cls_logits"),
          'roi_labels': t("post_labels"), 'rois': t("post_rois"), 'has_class_labels': True, 'cls_preds_normalized': False,
          'points': t("post_points"), 'gt_boxes': t("post_gt")}
    class_names = [str(n) for n in npz["post_class_names"]]
    padded = mu.post_processing_iou(bd, cfg, 3, class_names)
    pre = "post.%s." % variant
    assert np.allclose(padded['nms_scores'].cpu().numpy(), npz[pre + "nms_scores"], rtol=0, atol=1e-6)
    num = npz[pre + "num"]
    assert padded['num_pred'].cpu().tolist() == num.tolist()
    K = int(num.max())
    assert torch.equal(padded['pred_boxes'][:, :K].cpu(), torch.from_numpy(npz[pre + "pred_boxes"]))
    assert torch.equal(padded['pred_labels'][:, :K].cpu(), torch.from_numpy(npz[pre + "pred_labels"]))
    assert not padded['pred_boxes'][:, K:].any() and not padded['pred_labels'][:, K:].any()
    for key in ('pred_scores', 'pred_cls_scores', 'pred_iou_scores'):
        assert np.allclose(padded[key][:, :K].cpu().numpy(), npz[pre + key], rtol=0, atol=1e-6), key
    if variant == 'num_pts_iou_cls':
        from pdanet_amd.roiaware_pool3d_utils import points_in_boxes_count
        assert np.array_equal(points_in_boxes_count(bd['points'], bd['rois']).cpu().numpy(), npz["post_point_counts"])
    pred_dicts, recall = mu.to_iou_pred_and_recall_dicts(padded, cfg['RECALL_THRESH_LIST'])
    assert len(pred_dicts) == 2
    for s, d in enumerate(pred_dicts):
        assert set(d) == {'pred_boxes', 'pred_scores', 'pred_labels', 'pred_cls_scores', 'pred_iou_scores'}
        assert all(v.shape[0] == num[s] for v in d.values())
    assert list(recall) == [str(k) for k in npz[pre + "recall_keys"]] and [recall[k] for k in recall] == npz[pre + "recall_vals"].tolist()
    assert {'gt', 'roi_0.3', 'rcnn_0.3', 'roi_0.7', 'rcnn_0.7'} <= set(recall)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@gpu
def test_gpu_second_net_iou_train_and_eval():
    from pdanet_amd.second_net_iou import SECONDNetIoU
    from pdanet_amd.voxel_utils import VoxelGenerator, collate_voxels
    ds = CFG['dataset']
    B = 2
    torch.manual_seed(3)
    model = SECONDNetIoU(to_attr(CFG['MODEL']), 3, ds).cuda()
    rng = np.random.default_rng(5)
    pcr = np.array(ds['point_cloud_range'], np.float64)
    counts = [1500, 900]
    pts = np.concatenate([np.concatenate([rng.uniform(pcr[:3], pcr[3:], (n, 3)), rng.random((n, 1))], axis=1) for n in counts])
    offs = torch.tensor([0, counts[0], sum(counts)], dtype=torch.int64).cuda()
    gen = VoxelGenerator(ds['voxel_size'], ds['point_cloud_range'], 4, 5, 2000)
    voxels_, coords, num_points = collate_voxels(*gen.generate_batch((dev(pts.astype(np.float32)), offs, max(counts))))
    gt = np.zeros((B, 3, 8), np.float32)
    gt[0, 0] = [0.4, 0.0, -1.0, 3.9, 1.6, 1.56, 0.3, 1]
    gt[0, 1] = [0.3, 0.1, -0.6, 0.8, 0.6, 1.73, 1.2, 2]
    gt[1, 0] = [0.5, -0.1, -0.6, 1.76, 0.6, 1.73, -0.4, 3]
    roi_cfg = CFG['MODEL']['ROI_HEAD']
    n_rois, per_image = roi_cfg['NMS_CONFIG']['TRAIN']['NMS_POST_MAXSIZE'], roi_cfg['TARGET_CONFIG']['ROI_PER_IMAGE']
    # explicit draws, valid whatever the counts: the identity permutation of the foreground list, easy-background picks among
    # the zero-padded RoI rows, hard-background pick 0
    draws = {'perm': [np.arange(n_rois)] * B, 'fg_rand': rng.random((B, per_image)), 'hard_draw': np.zeros((B, per_image), np.int64),
             'easy_draw': rng.integers(0, n_rois - 16, (B, per_image))}
    batch = {'voxels': voxels_, 'voxel_coords': coords, 'voxel_num_points': num_points, 'gt_boxes': dev(gt), 'batch_size': B}
    model.train()
    ret, tb, disp = model(dict(batch, roi_target_draws=draws))
    assert torch.isfinite(ret['loss']) and disp == {}
    assert set(tb) == {'loss_rpn', 'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir', 'rpn_loss', 'rcnn_loss_iou', 'rcnn_loss'}
    assert float(ret['loss'].detach()) == pytest.approx(float(tb['loss_rpn'] + tb['rcnn_loss']), rel=1e-5)
    assert model.roi_head.forward_ret_dict['rcnn_iou'].shape == (B * per_image, 1)
    # the rcnn loss alone: a gradient on every roi_head parameter, none into the 2D backbone (the features are detached)
    loss_rcnn, _ = model.roi_head.get_loss()
    head_params, bev_params = list(model.roi_head.parameters()), list(model.backbone_2d.parameters())
    grads = torch.autograd.grad(loss_rcnn, head_params + bev_params, retain_graph=True, allow_unused=True)
    assert all(g is not None and torch.isfinite(g).all() for g in grads[:len(head_params)])
    assert all(g is None for g in grads[len(head_params):])
    ret['loss'].backward()
    for name, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    model.eval()
    with torch.no_grad():
        pred_dicts, recall = model(dict(batch, points=dev(np.concatenate([np.repeat(np.arange(B), counts)[:, None], pts], axis=1).astype(np.float32))))
    assert len(pred_dicts) == B
    assert set(pred_dicts[0]) == {'pred_boxes', 'pred_scores', 'pred_labels', 'pred_cls_scores', 'pred_iou_scores'}
    assert set(recall) == {'gt', 'roi_0.3', 'rcnn_0.3', 'roi_0.5', 'rcnn_0.5', 'roi_0.7', 'rcnn_0.7'}
    assert recall['gt'] == 3 and all(recall['roi_%s' % t] == recall['rcnn_%s' % t] for t in (0.3, 0.5, 0.7))
