"""PointIntraPartOffsetHead and its two entry points of csrc/parta2.hip (pdanet_amd/part_head.py): pda_part_assign_targets
against the reference's assign_stack_targets(ret_part_labels=True) (tests/golden/parta2.npz, written by make_parta2_golden.py
from the reference's own Python in float32 and in float64) and pda_part_loss against the torch composition of
get_part_layer_loss in float64.

Inputs (tests/golden/parta2_inputs.py): 2 scenes of 300 and 173 points, 4 boxes each with two overlapping ones and a
zero-padded row, every point at least 1e-3 m from every face of the boxes and of the enlarged boxes, so that the labels do not
depend on the arithmetic: the float32 and the float64 statement label all points alike, which is asserted on the inputs.

Tolerance (the rule of tests/test_second_net.py): max |a - ref| / max |ref| of the device against float64 may be FACTOR = 4
times that of the float32 CPU computation: the reference's float32 part labels for the targets, the float32 torch composition
for the loss and its gradient.  Both figures are printed; BASELINE.md section 4 records them."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pdanet_amd import _lib, build
from pdanet_amd.config import to_attr
from pdanet_amd.part_head import PointIntraPartOffsetHead, part_assign_targets, part_loss

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import parta2_inputs as inputs  # noqa: E402

gpu = pytest.mark.gpu
FACTOR = 4.0
with open(os.path.join(HERE, "golden", "parta2_state_dict.json")) as _f:
    FIXTURE = json.load(_f)
POINT_CFG = FIXTURE['config']['MODEL']['POINT_HEAD']
GOLD = np.load(os.path.join(HERE, "golden", "parta2.npz"))
DATA = inputs.part_head_inputs()


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_state_dict_is_the_references():
    head = PointIntraPartOffsetHead(num_class=1, input_channels=16, model_cfg=to_attr(POINT_CFG))
    own = head.state_dict()
    assert [[k, list(v.shape)] for k, v in own.items()] == FIXTURE['PointIntraPartOffsetHead']
    head.load_state_dict({k: torch.zeros(shape, dtype=own[k].dtype) for k, shape in FIXTURE['PointIntraPartOffsetHead']}, strict=True)
    assert head.box_layers is None and [n for n, _ in head.named_children()] == ['cls_loss_func', 'cls_layers', 'part_reg_layers']


def test_box_coder_is_refused_and_the_template_is_unchanged():
    cfg = json.loads(json.dumps(POINT_CFG))
    cfg['TARGET_CONFIG']['BOX_CODER'] = 'PointResidualCoder'
    with pytest.raises(NotImplementedError, match="BOX_CODER"):
        PointIntraPartOffsetHead(num_class=1, input_channels=16, model_cfg=to_attr(cfg))
    head = PointIntraPartOffsetHead(num_class=1, input_channels=16, model_cfg=to_attr(POINT_CFG))
    with pytest.raises(NotImplementedError):                                 # the template's own method still refuses
        head.assign_stack_targets(torch.zeros(2, 4), torch.zeros(1, 1, 8), ret_part_labels=True)


def test_inputs_hold_every_case_and_do_not_depend_on_the_arithmetic():
    assert GOLD['part_points'].tobytes() == DATA['points'].tobytes() and GOLD['part_gt_boxes'].tobytes() == DATA['gt_boxes'].tobytes()
    pts, gt = DATA['points'], DATA['gt_boxes']
    assert [int((pts[:, 0] == s).sum()) for s in (0, 1)] == [300, 173] and not gt[1, 3].any()
    for single, name in ((True, 'single'), (False, 'multi')):
        l32, _ = inputs.label_statement(pts, gt, DATA['extra_width'], np.float32, single)
        l64, p64 = inputs.label_statement(pts, gt, DATA['extra_width'], np.float64, single)
        assert np.array_equal(l32, l64)                                      # no point left out
        assert np.array_equal(l64, GOLD['part_labels_' + name]) and np.array_equal(l64, GOLD['part_labels_%s_f64' % name])
        fg = l64 > 0
        assert rel(p64[fg], GOLD['part_targets_%s_f64' % name][fg]) < 1e-12
        for s in (0, 1):
            here = pts[:, 0] == s
            assert (l64[here] > 0).any() and (l64[here] == -1).any() and (l64[here] == 0).any()
    assert set(np.unique(GOLD['part_labels_multi']).tolist()) == {-1, 0, 1, 2, 3}
    near_origin = np.abs(pts[:, 1:]).max(1) < 0.1                            # inside the enlarged zero-padded row only
    assert near_origin.sum() == 3 and (GOLD['part_labels_single'][near_origin] == -1).all()


def test_entry_points_exist_and_validate_before_any_launch(lib):
    i64, f3 = ctypes.c_int64, (ctypes.c_float * 3)(0.2, 0.2, 0.2)
    buf = ctypes.addressof((ctypes.c_double * 8)())
    err = lib.pda_last_error
    assert lib.pda_part_assign_targets(None, None, f3, None, None, i64(-1), 2, 4, 1, None) == 1 and b"bad size" in err()
    assert lib.pda_part_assign_targets(None, None, f3, None, None, i64(10), 0, 4, 1, None) == 1 and b"bad size" in err()
    assert lib.pda_part_assign_targets(None, None, f3, None, None, i64(10), 2, -1, 1, None) == 1 and b"bad size" in err()
    assert lib.pda_part_assign_targets(None, None, f3, None, None, i64(10), 2, 4, 1, None) == 1 and b"null" in err()
    assert lib.pda_part_assign_targets(buf + 4, buf, f3, buf, buf, i64(10), 2, 4, 1, None) == 1 and b"aligned" in err()
    assert lib.pda_part_assign_targets(None, None, f3, None, None, i64(0), 2, 4, 1, None) == 0          # no points: nothing to do
    assert lib.pda_part_loss(None, None, None, 1.0, None, None, None, i64(-1), None) == 1 and b"bad size" in err()
    assert lib.pda_part_loss(None, None, None, 1.0, None, buf, buf, i64(10), None) == 1 and b"null" in err()
    assert lib.pda_part_loss_blocks(i64(0)) == 1 and lib.pda_part_loss_blocks(i64(1)) == 1 and lib.pda_part_loss_blocks(i64(-1)) == -1
    assert lib.pda_part_loss_blocks(i64(1 << 30)) == 1024 and "pda_part_loss_blocks" in _lib.SIZE_QUERIES


def test_python_refuses_bad_shapes_and_cpu_tensors():
    with pytest.raises(ValueError):
        part_assign_targets(torch.zeros(4, 3), torch.zeros(1, 2, 8))
    with pytest.raises(ValueError):
        part_assign_targets(torch.zeros(4, 4), torch.zeros(1, 2, 7))
    with pytest.raises(RuntimeError, match="no CPU path"):
        part_assign_targets(torch.zeros(4, 4), torch.zeros(1, 2, 8))
    with pytest.raises(ValueError):
        part_loss(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(5, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        part_loss(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64))


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run_targets(points, gt, single):
    labels, part = part_assign_targets(dev(points), dev(gt), DATA['extra_width'], single)
    torch.cuda.synchronize()
    return labels.cpu().numpy(), part.cpu().numpy()


@gpu
@pytest.mark.parametrize("name", ["single", "multi"])
def test_gpu_targets_are_the_references(name):
    pts, gt = DATA['points'], DATA['gt_boxes']
    labels, part = run_targets(pts, gt, name == "single")
    assert labels.dtype == np.int64 and np.array_equal(labels, GOLD['part_labels_' + name])              # exactly the fixture's
    fg = labels > 0
    assert not part[~fg].any()                                                # exactly 0 off the foreground
    ref, f32 = GOLD['part_targets_%s_f64' % name][fg], GOLD['part_targets_' + name][fg]
    e_dev, e_f32 = rel(part[fg], ref), rel(f32, ref)
    print("part labels", name, "device err", e_dev, "float32 CPU err", e_f32)
    assert e_dev <= FACTOR * e_f32
    again = run_targets(pts, gt, name == "single")                           # two runs: the same bits
    assert again[0].tobytes() == labels.tobytes() and again[1].tobytes() == part.tobytes()


@gpu
def test_gpu_targets_with_an_empty_scene_shuffled_rows_and_stray_batch_values():
    pts, gt = DATA['points'], DATA['gt_boxes']
    labels, part = run_targets(pts, gt, False)
    # a scene with no points: the rows of scene 1 alone, then as scene 2 of three with an empty scene in between
    one = pts[:, 0] == 1
    l1, p1 = run_targets(pts[one], gt, False)
    assert np.array_equal(l1, labels[one]) and p1.tobytes() == part[one].tobytes()
    gt3 = np.concatenate([gt[:1], np.zeros_like(gt[:1]), gt[1:]])
    moved = pts.copy()
    moved[one, 0] = 2
    l3, p3 = run_targets(moved, gt3, False)
    assert np.array_equal(l3, labels) and p3.tobytes() == part.tobytes()
    # rows in shuffled order: every workgroup serves both scenes
    perm = np.random.default_rng(1).permutation(len(pts))
    ls, ps = run_targets(pts[perm], gt, False)
    assert np.array_equal(ls, labels[perm]) and ps.tobytes() == part[perm].tobytes()
    # a batch value outside [0, B), not an integer or not a number: label 0, part labels 0, the other rows untouched
    stray = pts.copy()
    hit = np.nonzero(labels > 0)[0][:4]
    stray[hit, 0] = [-1.0, 2.0, 0.5, np.nan]
    lx, px = run_targets(stray, gt, False)
    assert not lx[hit].any() and not px[hit].any()
    keep = np.ones(len(pts), bool)
    keep[hit] = False
    assert np.array_equal(lx[keep], labels[keep]) and px[keep].tobytes() == part[keep].tobytes()
    # no boxes at all
    l0, p0 = run_targets(pts, gt[:, :0], False)
    assert not l0.any() and not p0.any()


def composed_loss(logits, targets, labels, weight, dtype):
    """get_part_layer_loss (point_head_template.py:157-170) in torch on the CPU."""
    x = torch.tensor(logits, dtype=dtype, requires_grad=True)
    t, pos = torch.tensor(targets, dtype=dtype), torch.tensor(labels) > 0
    loss = F.binary_cross_entropy(torch.sigmoid(x), t, reduction='none')
    loss = (loss.sum(dim=-1) * pos.to(dtype)).sum() / (3 * max(1, int(pos.sum()))) * weight
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


@gpu
def test_gpu_part_loss_and_its_gradient():
    logits, targets, labels = GOLD['part_logits'], GOLD['part_targets_single'], GOLD['part_labels_single']
    assert logits.min() < -9 and logits.max() > 9 and np.abs(logits).max() <= 10
    weight = 1.5
    x = dev(logits).requires_grad_(True)
    loss, out = part_loss(x, dev(targets), dev(labels), weight)
    (loss * 2.0).backward()
    torch.cuda.synchronize()
    ref_loss, ref_grad = composed_loss(logits, targets, labels, weight, torch.float64)
    f32_loss, f32_grad = composed_loss(logits, targets, labels, weight, torch.float32)
    e_dev, e_f32 = abs(float(loss.detach()) - ref_loss) / abs(ref_loss), abs(f32_loss - ref_loss) / abs(ref_loss)
    print("part loss device err", e_dev, "float32 CPU err", e_f32)
    g_dev, g_f32 = rel(x.grad.cpu().numpy() / 2.0, ref_grad), rel(f32_grad, ref_grad)
    print("part loss gradient device err", g_dev, "float32 CPU err", g_f32)
    assert e_dev <= FACTOR * e_f32 and g_dev <= FACTOR * g_f32
    assert int(out[2]) == int((labels > 0).sum()) and float(out[0]) == float(loss.detach())
    assert abs(float(GOLD['part_loss']) * weight - ref_loss) / ref_loss < 1e-5                           # the reference's own float32 loss
    x2 = dev(logits).requires_grad_(True)                                    # two runs: the same bits
    loss2, _ = part_loss(x2, dev(targets), dev(labels), weight)
    (loss2 * 2.0).backward()
    assert torch.equal(loss, loss2) and torch.equal(x.grad, x2.grad)


@gpu
def test_gpu_part_loss_without_positives_and_at_the_clamp():
    logits, targets = GOLD['part_logits'], GOLD['part_targets_single']
    x = dev(logits).requires_grad_(True)
    loss, out = part_loss(x, dev(targets), torch.zeros(len(logits), dtype=torch.int64, device='cuda'))
    loss.backward()
    assert float(loss) == 0.0 and float(out[2]) == 0.0 and torch.isfinite(x.grad).all() and not x.grad.any()
    # logits far outside: log(sigmoid) is clamped at -100 as torch clamps it, loss and gradient stay finite
    big = torch.tensor([[-300.0, 300.0, 0.0]], device='cuda', requires_grad=True)
    loss, _ = part_loss(big, torch.tensor([[1.0, 0.0, 0.5]], device='cuda'), torch.ones(1, dtype=torch.int64, device='cuda'))
    loss.backward()
    want = (100.0 + 100.0 + float(np.log(2.0))) / 3
    assert abs(float(loss) - want) < 1e-5 * want and torch.isfinite(big.grad).all()
    # no rows at all
    loss, out = part_loss(torch.zeros(0, 3, device='cuda'), torch.zeros(0, 3, device='cuda'), torch.zeros(0, dtype=torch.int64, device='cuda'))
    assert float(loss) == 0.0


@gpu
def test_gpu_head_forward_loss_and_backward():
    torch.manual_seed(0)
    head = PointIntraPartOffsetHead(num_class=1, input_channels=16, model_cfg=to_attr(POINT_CFG)).cuda().train()
    pts = DATA['points']
    batch = {'batch_size': 2, 'point_features': torch.randn(len(pts), 16, device='cuda'), 'point_coords': dev(pts),
             'gt_boxes': dev(DATA['gt_boxes'])}
    out = head(batch)
    assert out['point_cls_scores'].shape == (len(pts),) and out['point_part_offset'].shape == (len(pts), 3)
    ret = head.forward_ret_dict
    assert np.array_equal(ret['point_cls_labels'].cpu().numpy(), GOLD['part_labels_single']) and ret['point_box_labels'] is None
    loss, tb = head.get_loss()
    assert set(tb) == {'point_loss_cls', 'point_pos_num', 'point_loss_part'}
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 0 for v in tb.values())       # nothing read back
    loss.backward()
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in head.parameters())
    # the part term against the torch composition on the same predictions
    ref, _ = composed_loss(ret['point_part_preds'].detach().cpu().numpy(), GOLD['part_targets_single_f64'], GOLD['part_labels_single'],
                           POINT_CFG['LOSS_CONFIG']['LOSS_WEIGHTS']['point_part_weight'], torch.float64)
    assert abs(float(tb['point_loss_part']) - ref) < 1e-5 * abs(ref)
    head.eval()
    with torch.no_grad():
        head(dict(batch))
    assert 'point_cls_labels' not in head.forward_ret_dict
