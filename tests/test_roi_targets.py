"""The RoI-head front end (csrc/roi_targets.hip, pdanet_amd/proposal_target_layer.py, roi_head_template.py, ResidualCoder)
against tests/golden/roi_targets.npz, the reference's RoIHeadTemplate / ProposalTargetLayer run on CPU tensors
(tests/golden/make_roi_targets_golden.py)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import roi_targets_cover as cover  # noqa: E402

LOSS_WEIGHTS = {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0, 'code_weights': [1.0] * 7}
TARGET_KEYS = ('rois', 'gt_of_rois', 'gt_iou_of_rois', 'roi_scores', 'roi_labels', 'reg_valid_mask', 'rcnn_cls_labels',
               'gt_of_rois_src')


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "roi_targets.npz"))


@pytest.fixture(scope="module")
def lib():
    from pdanet_amd import build, _lib
    build.build()
    return _lib.load()


def _batches(fx):
    out = []
    for i in range(int(fx['n_batches'])):
        p = 'b%d_' % i
        b = {k[len(p):]: fx[k] for k in fx.files if k.startswith(p)}
        b['case'], b['cfg'] = str(b['case']), json.loads(str(b['cfg']))
        out.append(b)
    return out


def _model_cfg(target_cfg, loss_cfg=None):
    from pdanet_amd.config import to_attr
    loss_cfg = loss_cfg or {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                            'LOSS_WEIGHTS': LOSS_WEIGHTS}
    return to_attr({'TARGET_CONFIG': dict(target_cfg, BOX_CODER='ResidualCoder'), 'DP_RATIO': 0.3, 'LOSS_CONFIG': loss_cfg})


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def _max_iou(lib, b=2, m=64, t=8, cols=8, by_class=1, ptr=None):
    return lib.pda_roi_max_iou(ptr, ptr, ptr, cols, by_class, ptr, ptr, b, m, t, None)


def _sample(lib, b=2, m=64, t=8, cols=8, r=32, fg=16, ratio=0.8, score=0, ptr=None, draws=(None,) * 4):
    d = ctypes.c_double
    return lib.pda_roi_sample_targets(ptr, ptr, ptr, ptr, cols, ptr, ptr, r, fg, d(ratio), d(0.55), d(0.6), d(0.45), d(0.1), score,
                                      *draws, ctypes.c_uint64(1), *([ptr] * 10), b, m, t, None)


def test_argument_validation_without_gpu(lib):
    """Sizes are refused before any pointer is used or anything is launched; empty problems are PDA_OK and touch nothing."""
    err = lib.pda_last_error
    for fn in (_max_iou, _sample):
        assert fn(lib, b=-1) == 1 and fn(lib, m=-1) == 1 and fn(lib, t=-1) == 1
        assert fn(lib, cols=7) == 1 and b"gt_cols" in err()
        assert fn(lib, m=1024) == 1 and b"null" in err()                  # a supported size: only the pointers are missing
        assert fn(lib, m=4096) == 1 and b"null" in err()
        assert fn(lib, m=4097) == 1 and b"m=4097" in err()
        assert fn(lib, b=65536) == 1
        assert fn(lib) == 1 and b"null" in err()
        assert fn(lib, b=0) == 0 and fn(lib, m=0) == 0                    # the empty problem
    assert _sample(lib, r=0) == 1 and b"roi_per_image" in err()
    assert _sample(lib, r=-3) == 1
    assert _sample(lib, r=0, b=0) == 1                                    # also for an empty batch
    assert _sample(lib, fg=33) == 1 and _sample(lib, fg=-1) == 1
    assert _sample(lib, ratio=1.5) == 1 and _sample(lib, score=2) == 1
    one = ctypes.cast((ctypes.c_int64 * 1)(), ctypes.c_void_p)
    assert _sample(lib, ptr=one, draws=(one, None, None, None)) == 1 and b"explicit draws" in err()
    assert _sample(lib, t=0) == 1 and b"null" in err()                    # t == 0 is a real problem (one zero box), not empty


def test_fixture_covers_cases(fx):
    seen, shapes = cover.coverage(fx)
    assert not cover.REQUIRED - seen, sorted(cover.REQUIRED - seen)
    for k, want in cover.SHAPES.items():
        assert shapes[k] <= want and len(shapes[k]) >= 2, (k, shapes[k])
    assert os.path.getsize(os.path.join(HERE, "golden", "roi_targets.npz")) < 1 << 20
    for b in _batches(fx):                               # the draws are stored for the branch every scene takes
        R = b['cfg']['ROI_PER_IMAGE']
        for s in range(b['rois'].shape[0]):
            fg, hard, easy = (int(m.sum()) for m in cover.category_counts(b['max_overlaps'][s], b['cfg']))
            p_fg, p_hard, p_easy = cover.pick_counts(fg, hard, easy, b['cfg'])
            both = fg > 0 and hard + easy > 0
            assert list(b['draw_counts'][s]) == [fg if both else 0, R if fg and not both else 0, p_hard, p_easy]
            assert sorted(b['perm'][s, :fg]) == list(range(fg)) or not both
            assert p_fg + p_hard + p_easy == R


def test_residual_coder_matches_reference(fx):
    import torch
    from pdanet_amd.box_coder_utils import ResidualCoder
    boxes, anchors = torch.from_numpy(fx['coder_boxes']), torch.from_numpy(fx['coder_anchors'])
    for tag, sincos in (('res', False), ('sincos', True)):
        coder = ResidualCoder(encode_angle_by_sincos=sincos)
        assert coder.code_size == (8 if sincos else 7)
        b0, a0 = boxes.clone(), anchors.clone()
        codes = coder.encode_torch(boxes, anchors)
        assert torch.equal(boxes, b0) and torch.equal(anchors, a0)        # the reference's clamps its arguments in place
        ref = torch.from_numpy(fx['coder_%s_codes' % tag])
        assert codes.shape == ref.shape and (codes - ref).abs().max() <= 2e-6 * max(1.0, ref.abs().max())
        clamped = anchors.clone()
        clamped[:, 3:6] = clamped[:, 3:6].clamp(min=1e-5)
        dec = coder.decode_torch(ref, clamped)
        ref_dec = torch.from_numpy(fx['coder_%s_decoded' % tag])
        assert (dec - ref_dec).abs().max() <= 2e-6 * max(1.0, ref_dec.abs().max())
        if not sincos:                                   # decode(encode(x)) == x; row 0's anchor size sits below the clamp
            assert (coder.decode_torch(codes, clamped)[1:] - boxes[1:]).abs().max() <= 1e-4
        else:                                            # the heading comes back modulo 2 pi
            back = coder.decode_torch(codes, clamped)[1:]
            assert (back[:, :6] - boxes[1:, :6]).abs().max() <= 1e-4
            d = (back[:, 6] - boxes[1:, 6] + np.pi) % (2 * np.pi) - np.pi
            assert d.abs().max() <= 1e-4


def test_fc_layers_have_the_reference_state_dict_keys(fx):
    from pdanet_amd.roi_head_template import RoIHeadTemplate
    head = RoIHeadTemplate(3, _model_cfg(_batches(fx)[0]['cfg']))
    fc = head.make_fc_layers(input_channels=128, output_channels=7, fc_list=[256, 256])
    assert list(fc.state_dict().keys()) == [str(k) for k in fx['fc_keys']]
    assert [type(m).__name__ for m in fc] == [str(k) for k in fx['fc_modules']]


def test_unknown_score_type_and_wide_boxes_are_refused(fx):
    import torch
    from pdanet_amd.proposal_target_layer import ProposalTargetLayer, roi_max_iou
    cfg = dict(_batches(fx)[0]['cfg'], CLS_SCORE_TYPE='raw_roi_iou')
    with pytest.raises(NotImplementedError):
        ProposalTargetLayer(cfg)
    with pytest.raises(NotImplementedError, match="boxes with velocities are not supported"):
        roi_max_iou(torch.zeros(1, 4, 9), torch.zeros(1, 4, dtype=torch.long), torch.zeros(1, 2, 10))
    with pytest.raises(RuntimeError, match="no CPU path"):
        roi_max_iou(torch.zeros(1, 4, 7), torch.zeros(1, 4, dtype=torch.long), torch.zeros(1, 2, 8))


def _loss_case(fx, i, device='cpu'):
    import torch
    from pdanet_amd.roi_head_template import RoIHeadTemplate
    p = 'l%d_' % i
    b = _batches(fx)[int(fx[p + 'batch'])]
    head = RoIHeadTemplate(3, _model_cfg(b['cfg'], json.loads(str(fx[p + 'loss_cfg'])))).to(device)
    rcnn_cls = torch.from_numpy(fx[p + 'rcnn_cls']).to(device).requires_grad_(True)
    rcnn_reg = torch.from_numpy(fx[p + 'rcnn_reg']).to(device).requires_grad_(True)
    fr = {k: torch.from_numpy(b['t_' + k]).to(device) for k in TARGET_KEYS}
    return head, fr, rcnn_cls, rcnn_reg, p


def _check_loss(fx, i, device):
    """Loss terms and gradients within the head's bound (2e-5)."""
    import torch
    head, fr, rcnn_cls, rcnn_reg, p = _loss_case(fx, i, device)
    before = {k: v.clone() for k, v in fr.items()}
    head.forward_ret_dict = dict(fr, rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg)
    loss, tb = head.get_loss()
    loss.backward()
    assert all(torch.equal(fr[k], before[k]) for k in fr)                 # the targets are not written into
    ref_tb = dict(zip((str(k) for k in fx[p + 'tb_keys']), fx[p + 'tb_vals']))
    assert set(tb) == set(ref_tb)
    for k, v in ref_tb.items():
        assert isinstance(tb[k], torch.Tensor) and tb[k].dim() == 0 and not tb[k].requires_grad
        print(p, k, float(tb[k]), float(v))
        assert float(tb[k]) == pytest.approx(float(v), rel=2e-5, abs=1e-6), k
    assert float(loss.detach()) == pytest.approx(float(fx[p + 'loss']), rel=2e-5)
    for g, ref in ((rcnn_cls.grad, fx[p + 'grad_cls']), (rcnn_reg.grad, fx[p + 'grad_reg'])):
        err = np.abs(g.cpu().numpy() - ref).max()
        print(p, 'grad', err, np.abs(ref).max())
        assert err <= 2e-5 * max(1.0, np.abs(ref).max())
    with torch.no_grad():
        bc, bb = head.generate_predicted_boxes(fr['rois'].shape[0], fr['rois'], rcnn_cls.detach(), rcnn_reg.detach())
    assert torch.equal(bc.cpu(), torch.from_numpy(fx[p + 'pred_cls']))
    ref = fx[p + 'pred_boxes']
    assert bb.shape == ref.shape and np.abs(bb.cpu().numpy() - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("i", range(4))
def test_get_loss_and_predicted_boxes_match_reference_cpu(fx, i):
    _check_loss(fx, i, 'cpu')


def test_cls_targets_with_binary_cross_entropy_cpu(fx):
    """PointRCNN's pairing ('cls' targets with their -1, BinaryCrossEntropy): the ignored rows carry no loss and no gradient."""
    import torch
    import torch.nn.functional as F
    from pdanet_amd.roi_head_template import RoIHeadTemplate
    b = _batches(fx)[0]
    head = RoIHeadTemplate(3, _model_cfg(b['cfg']))
    labels = torch.from_numpy(b['t_rcnn_cls_labels'])
    assert (labels == -1).any() and (labels == 1).any() and (labels == 0).any()
    x = torch.linspace(-3, 3, labels.numel()).view(-1, 1).requires_grad_(True)
    loss, tb = head.get_box_cls_layer_loss({'rcnn_cls': x, 'rcnn_cls_labels': labels})
    loss.backward()
    valid = labels.view(-1) >= 0
    ref = F.binary_cross_entropy_with_logits(x.detach().view(-1)[valid], labels.view(-1)[valid].float(), reduction='sum') / valid.sum()
    assert float(loss) == pytest.approx(float(ref), rel=1e-5)
    assert (x.grad.view(-1)[~valid] == 0).all() and x.grad.view(-1)[valid].abs().min() > 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _dev(b, keys=('rois', 'roi_scores', 'roi_labels', 'gt_boxes')):
    import torch
    return {k: torch.from_numpy(b[k]).cuda() for k in keys}


def _draws(b):
    return {k: b[k] for k in ('perm', 'fg_rand', 'hard_draw', 'easy_draw')}


@pytest.mark.gpu
def test_max_iou_is_bit_identical_to_the_reference(fx):
    import torch
    from pdanet_amd import iou3d_nms_utils
    from pdanet_amd.proposal_target_layer import roi_max_iou
    for b in _batches(fx):
        d = _dev(b)
        by_class = bool(b['cfg']['SAMPLE_ROI_BY_EACH_CLASS'])
        mo, ga = roi_max_iou(d['rois'], d['roi_labels'], d['gt_boxes'], by_class=by_class)
        assert mo.dtype == torch.float32 and ga.dtype == torch.int32
        assert np.array_equal(mo.cpu().numpy().view(np.uint32), b['max_overlaps'].view(np.uint32)), b['case']
        assert np.array_equal(ga.cpu().numpy(), b['gt_assignment']), b['case']
        # and to this library's boxes_iou3d_gpu on the trimmed GT, class-agnostic
        mo_a, ga_a = roi_max_iou(d['rois'], d['roi_labels'], d['gt_boxes'], by_class=False)
        for s in range(b['rois'].shape[0]):
            kept = cover.kept_rows(b['gt_boxes'][s])
            v, i = iou3d_nms_utils.boxes_iou3d_gpu(d['rois'][s], d['gt_boxes'][s, :kept, :7]).cpu().max(dim=1)   # CPU max: the first
            assert torch.equal(mo_a[s].cpu().view(torch.int32), v.view(torch.int32)), (b['case'], s)
            assert torch.equal(ga_a[s].cpu().long(), i), (b['case'], s)


def _rotated_offset_bound(b):
    """Per element of gt_of_rois[..., 0:2]: (|dx| + |dy|) 2^-21 + 2 spacing(max(|dx|, |dy|)), dx, dy the offset before the
    rotation.  Both sides take sin and cos of the identical float32 angle, each within 2 ulp of the true value, so they
    differ by at most 4 * 2^-24 absolute, which scales the two operands; the two products and the sum add at most two
    roundings at the operands' magnitude; the bound is twice that."""
    dx = np.abs(b['t_gt_of_rois_src'][..., 0] - b['t_rois'][..., 0]).astype(np.float32)
    dy = np.abs(b['t_gt_of_rois_src'][..., 1] - b['t_rois'][..., 1]).astype(np.float32)
    return ((dx + dy).astype(np.float64) * 2.0 ** -21 + 2 * np.spacing(np.maximum(dx, dy)).astype(np.float64))[..., None]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.gpu
def test_explicit_draws_reproduce_the_reference_targets(fx):
    import torch
    from pdanet_amd.proposal_target_layer import ProposalTargetLayer
    for b in _batches(fx):
        layer = ProposalTargetLayer(b['cfg'])
        d = _dev(b)
        t = layer(dict(d, batch_size=b['rois'].shape[0]), draws=_draws(b), check=True)
        assert not t['status'].any()
        got = {k: v.cpu().numpy() for k, v in t.items()}
        for k in ('rois', 'roi_scores', 'roi_labels', 'gt_iou_of_rois', 'gt_of_rois_src', 'reg_valid_mask', 'rcnn_cls_labels'):
            ref = b['t_' + k]
            assert got[k].dtype == ref.dtype and got[k].shape == ref.shape, (b['case'], k)
            assert np.array_equal(_bits(got[k]), _bits(ref)), (b['case'], k)
        # the sampled indices: every output row is a RoI of the scene with that box and that IoU, and it is the one picked
        for s in range(b['rois'].shape[0]):
            for r in range(got['rois'].shape[1]):
                cand = np.flatnonzero((b['rois'][s] == b['t_rois'][s, r]).all(axis=1) &
                                      (b['max_overlaps'][s] == b['t_gt_iou_of_rois'][s, r]))
                assert got['sampled_inds'][s, r] in cand, (b['case'], s, r)
        ref = b['t_gt_of_rois']
        assert np.array_equal(_bits(got['gt_of_rois'][..., 2:]), _bits(ref[..., 2:])), b['case']   # z, sizes, folded heading, label
        err = np.abs(got['gt_of_rois'][..., :2].astype(np.float64) - ref[..., :2].astype(np.float64))
        bound = _rotated_offset_bound(b)
        print(b['case'], 'rotated offset: max err / bound', (err / np.maximum(bound, 1e-300)).max())
        assert (err <= bound).all(), b['case']


def _check_seeded_invariants(b, t):
    got = {k: v.cpu().numpy() for k, v in t.items()}
    assert not got['status'].any()
    for s in range(b['rois'].shape[0]):
        masks = cover.category_counts(b['max_overlaps'][s], b['cfg'])
        n = [int(m.sum()) for m in masks]
        p_fg, p_hard, p_easy = cover.pick_counts(*n, b['cfg'])
        inds = got['sampled_inds'][s]
        for lo, hi, mask in ((0, p_fg, masks[0]), (p_fg, p_fg + p_hard, masks[1]), (p_fg + p_hard, p_fg + p_hard + p_easy, masks[2])):
            assert mask[inds[lo:hi]].all(), (b['case'], s)                # every pick lies in its category list
        if n[1] + n[2] > 0:
            assert len(set(inds[:p_fg])) == p_fg                          # without replacement when bg exists
        assert np.array_equal(got['rois'][s], b['rois'][s][inds]) and np.array_equal(got['gt_iou_of_rois'][s], b['max_overlaps'][s][inds])
        assert np.array_equal(got['roi_labels'][s], b['roi_labels'][s][inds])
    return got['sampled_inds']


@pytest.mark.gpu
def test_seeded_mode_keeps_the_branch_rules(fx):
    import torch
    from pdanet_amd.proposal_target_layer import ProposalTargetLayer
    for b in _batches(fx):
        layer = ProposalTargetLayer(b['cfg'])
        bd = dict(_dev(b), batch_size=b['rois'].shape[0])
        t1, t2, t3 = layer(bd, seed=1234), layer(bd, seed=1234), layer(bd, seed=99)
        for k in t1:
            assert torch.equal(t1[k], t2[k]), (b['case'], k)              # the same seed, the same outputs
        i1 = _check_seeded_invariants(b, t1)
        i3 = _check_seeded_invariants(b, t3)
        if b['case'] == 'pointrcnn':
            assert not np.array_equal(i1, i3)
    torch.manual_seed(5)                                 # without a seed: torch's CPU generator
    a = layer(bd)
    torch.manual_seed(5)
    assert torch.equal(a['sampled_inds'], layer(bd)['sampled_inds'])


@pytest.mark.gpu
def test_nan_scene_sets_status_and_leaves_the_others_alone(fx, monkeypatch):
    import torch
    from pdanet_amd.proposal_target_layer import roi_sample_targets, ProposalTargetLayer
    b = _batches(fx)[2]
    d = _dev(b)
    mo, ga = torch.from_numpy(b['max_overlaps']).cuda(), torch.from_numpy(b['gt_assignment']).cuda()
    good = roi_sample_targets(d['rois'], d['roi_scores'], d['roi_labels'], d['gt_boxes'], mo, ga, b['cfg'], seed=3)
    mo_nan = mo.clone()
    mo_nan[1] = float('nan')
    bad = roi_sample_targets(d['rois'], d['roi_scores'], d['roi_labels'], d['gt_boxes'], mo_nan, ga, b['cfg'], seed=3)
    assert bad['status'].tolist() == [0, 1, 0, 0] and good['status'].tolist() == [0, 0, 0, 0]
    for k in TARGET_KEYS:
        assert not bad[k][1].any(), k                    # the scene's rows are zero
        for s in (0, 2, 3):
            assert torch.equal(bad[k][s], good[k][s]), (k, s)
    # through the layer: check=True reads status and raises as the reference does, check=False reads nothing
    import pdanet_amd.proposal_target_layer as ptl
    monkeypatch.setattr(ptl, "roi_max_iou", lambda *a, **k: (mo_nan, ga))
    layer = ProposalTargetLayer(b['cfg'])
    bd = dict(d, batch_size=4)
    assert layer(bd, seed=3, check=False)['status'].tolist() == [0, 1, 0, 0]
    with pytest.raises(NotImplementedError):
        layer(bd, seed=3, check=True)


def _proposal_case(fx, i):
    import torch
    from pdanet_amd.config import to_attr
    p = 'p%d_' % i
    cfg = to_attr(json.loads(str(fx[p + 'nms_cfg'])))
    box, cls = torch.from_numpy(fx[p + 'box_preds']).cuda(), torch.from_numpy(fx[p + 'cls_preds']).cuda()
    bd = {'batch_size': box.shape[0], 'cls_preds_normalized': False, 'gt_boxes': torch.from_numpy(fx[p + 'gt_boxes']).cuda()}
    if str(fx[p + 'layout']) == '3d':
        bd.update(batch_box_preds=box, batch_cls_preds=cls)
    else:
        B, N = box.shape[:2]
        bd.update(batch_box_preds=box.view(B * N, -1), batch_cls_preds=cls.view(B * N, -1),
                  batch_index=torch.arange(B, device='cuda').repeat_interleave(N).float())
    return bd, cfg, p


@pytest.mark.gpu
def test_proposal_layer_matches_reference_in_both_layouts(fx):
    import torch
    from pdanet_amd.roi_head_template import RoIHeadTemplate
    head = RoIHeadTemplate(3, _model_cfg(_batches(fx)[0]['cfg']))
    for i in range(int(fx['n_proposal'])):
        bd, cfg, p = _proposal_case(fx, i)
        out = head.proposal_layer(bd, cfg)
        assert out['has_class_labels'] is True and 'batch_index' not in out
        for k in ('rois', 'roi_scores', 'roi_labels'):
            ref = fx[p + k]
            got = out[k].cpu().numpy()
            assert got.shape == ref.shape and got.dtype == ref.dtype and np.array_equal(_bits(got), _bits(ref)), (i, k)
        pad = ~fx[p + 'rois'].any(axis=2)
        assert (out['roi_labels'].cpu().numpy()[pad] == 1).all()
        rois = out['rois']
        again = head.proposal_layer(out, cfg)            # rois present: returned untouched
        assert again is out and again['rois'] is rois
    with pytest.raises(NotImplementedError):
        head.proposal_layer(_proposal_case(fx, 0)[0], dict(cfg, MULTI_CLASSES_NMS=True))


@pytest.mark.gpu
def test_proposals_to_targets_replay_in_one_graph(fx):
    """proposal_layer -> assign_targets (seeded, check=False) holds no host read: it is captured in one graph on a side
    stream after a warm-up call, the inputs are overwritten with a second batch of the same shapes, and one replay equals
    the eager result for that batch."""
    import torch
    from pdanet_amd.roi_head_template import RoIHeadTemplate
    head = RoIHeadTemplate(3, _model_cfg(dict(_batches(fx)[0]['cfg'], ROI_PER_IMAGE=32)))
    bd0, cfg, _ = _proposal_case(fx, 0)
    bd2, _, _ = _proposal_case(fx, 2)
    keys = ('batch_box_preds', 'batch_cls_preds', 'gt_boxes')
    assert all(bd0[k].shape == bd2[k].shape for k in keys)

    def run(bd):
        return head.assign_targets(head.proposal_layer(dict(bd), cfg), seed=77, check=False)

    eager0, eager2 = run(bd0), run(bd2)
    assert not torch.equal(eager0['rois'], eager2['rois'])
    static = {k: bd0[k].clone() for k in keys}
    static.update(batch_size=bd0['batch_size'], cls_preds_normalized=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)                                      # warm-up
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = run(static)
    torch.cuda.current_stream().wait_stream(side)
    for k in keys:
        static[k].copy_(bd2[k])
    g.replay()
    torch.cuda.synchronize()
    for k in eager2:
        assert torch.equal(out[k], eager2[k]), k


@pytest.mark.gpu
def test_sampled_rois_feed_roipoint_pool3d(fx):
    """End to end at small size: B 2, M 128, R 32, 2048 points a scene, 64 sampled points; the empty flags are what the
    points_in_boxes counts of the enlarged boxes say."""
    import torch
    from pdanet_amd import box_utils
    from pdanet_amd.proposal_target_layer import ProposalTargetLayer
    from pdanet_amd.roipoint_pool3d_utils import RoIPointPool3d
    from pdanet_amd.roiaware_pool3d_utils import points_in_boxes_cpu
    b = next(x for x in _batches(fx) if x['case'] == 'overlap')
    d = {k: v[:2].contiguous() for k, v in _dev(b).items()}
    t = ProposalTargetLayer(b['cfg'])(dict(d, batch_size=2), seed=11)
    rois = t['rois']
    assert rois.shape == (2, 32, 7)
    gen = torch.Generator().manual_seed(0)
    # points scattered around the GT boxes of each scene, so that some RoIs hold points and some do not
    centres = d['gt_boxes'][:, :8, :3].cpu()
    pts = centres[:, torch.randint(0, 8, (2048,), generator=gen)] + torch.randn(2, 2048, 3, generator=gen) * 1.5
    pts = pts.cuda().contiguous()
    feats = torch.randn(2, 2048, 16, generator=gen).cuda()
    pool = RoIPointPool3d(num_sampled_points=64, pool_extra_width=1.0)
    pooled, empty = pool(pts, feats, rois)
    assert pooled.shape == (2, 32, 64, 3 + 16) and empty.shape == (2, 32)
    enlarged = box_utils.enlarge_box3d(rois.view(-1, 7), (1.0, 1.0, 1.0)).view(2, 32, 7)
    counts = torch.stack([points_in_boxes_cpu(pts[s], enlarged[s]).sum(dim=-1) for s in range(2)])
    assert torch.equal(empty.bool().cpu(), (counts == 0).cpu())
    assert empty.any() and not empty.all()


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 1])
def test_get_loss_on_the_device_reads_nothing(fx, i):
    import torch
    _check_loss(fx, i, 'cuda')
    head, fr, rcnn_cls, rcnn_reg, _ = _loss_case(fx, i, 'cuda')
    head.forward_ret_dict = dict(fr, rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg)
    torch.cuda.set_sync_debug_mode(2)                    # a synchronising call raises
    try:
        loss, tb = head.get_loss()
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
