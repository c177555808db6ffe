"""ONCE evaluation on the device (csrc/once_eval.hip, pdanet_amd/once_eval.py) against tests/golden/once_eval.npz, which
holds the reference's own evaluation.py / iou_utils.py run on synthetic frames (make_once_eval_golden.py)."""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "once_eval.npz")
CONFIGS = {
    'default': {},
    'no_superclass': {'use_superclass': False},
    'overall': {'difficulty_mode': 'Overall'},
    'distance': {'difficulty_mode': 'Distance'},
    'no_heading': {'ap_with_heading': False},
    'pr40': {'num_pr_points': 40},
}


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _annos(g):
    names = [str(n) for n in g['names']]
    go = np.concatenate([[0], np.cumsum(g['gt_count'])])
    po = np.concatenate([[0], np.cumsum(g['pred_count'])])
    gt, pred = [], []
    for f in range(len(g['gt_count'])):
        gt.append({'name': np.array([names[i] for i in g['gt_name'][go[f]:go[f + 1]]], dtype='<U10'),
                   'boxes_3d': g['gt_boxes'][go[f]:go[f + 1]]})
        if po[f + 1] == po[f]:
            pred.append({'name': np.zeros(0), 'score': np.zeros(0), 'boxes_3d': np.zeros((0, 7))})
        else:
            pred.append({'name': np.array([names[i] for i in g['pred_name'][po[f]:po[f + 1]]]),
                         'score': g['pred_score'][po[f]:po[f + 1]], 'boxes_3d': g['pred_boxes'][po[f]:po[f + 1]]})
    return gt, pred


@pytest.fixture(scope="module")
def lib():
    from pdanet_amd import build, _lib
    build.build()
    return _lib.load()


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_capi_argument_validation(lib):
    from pdanet_amd import _lib
    assert lib.pda_once_eval_workspace_bytes(-1, 10, 4) == -1
    assert lib.pda_once_eval_workspace_bytes(3, 10, 0) == -1
    assert lib.pda_once_eval_workspace_bytes(3, 10, 65) == -1
    assert lib.pda_once_eval_workspace_bytes(3, 10, 12) >= 12 * 10 * 4 + 12 * 8
    assert lib.pda_once_eval_workspace_bytes(0, 0, 1) >= 8
    st = lib.pda_once_eval_iou(None, 1, None, None, None)
    assert st != 0 and b"null frames" in lib.pda_last_error()
    fr = _lib.OnceFrames(n_frames=2, max_gt=4, max_pred=5000)
    st = lib.pda_once_eval_iou(ctypes.byref(fr), 1, None, None, None)
    assert st != 0 and b"max_pred" in lib.pda_last_error()
    fr = _lib.OnceFrames(n_frames=-1)
    assert lib.pda_once_eval_iou(ctypes.byref(fr), 1, None, None, None) != 0
    fr = _lib.OnceFrames(n_frames=2, max_gt=4, max_pred=8)                # frame arrays missing
    st = lib.pda_once_eval_iou(ctypes.byref(fr), 1, None, None, None)
    assert st != 0 and b"null frame arrays" in lib.pda_last_error()
    fr0 = _lib.OnceFrames(n_frames=0)
    acc = (ctypes.c_uint8 * 64)(*([1] * 64))
    thr = (ctypes.c_double * 17)(*([0.5] * 17))
    args = lambda n_cls, n_names, mode: (ctypes.byref(fr0), None, acc, n_cls, n_names, thr, mode)
    for bad, msg in [((17, 4, 0), b"n_classes"), ((0, 4, 0), b"n_classes"), ((3, 65, 0), b"n_names"),
                     ((3, 4, 3), b"difficulty_mode"), ((3, 4, -1), b"difficulty_mode")]:
        assert lib.pda_once_eval_accumulate(*args(*bad), None, None, None, None) != 0
        assert msg in lib.pda_last_error()
        assert lib.pda_once_eval_match(*args(*bad), 50, None, None, None, None, None, None, None, None) != 0
    neg = (ctypes.c_double * 3)(0.7, -0.1, 0.5)
    assert lib.pda_once_eval_accumulate(ctypes.byref(fr0), None, acc, 3, 4, neg, 0, None, None, None, None) != 0
    assert b"< 0" in lib.pda_last_error()
    st = lib.pda_once_eval_match(*args(3, 4, 0), 0, None, None, None, None, None, None, None, None)
    assert st != 0 and b"num_pr_points" in lib.pda_last_error()
    st = lib.pda_once_eval_match(*args(3, 4, 0), 50, None, None, None, None, None, None, None, None)
    assert st != 0 and b"null workspace" in lib.pda_last_error()


def test_accept_table_superclass_and_plain():
    from pdanet_amd import once_eval as oe
    names = ['Car', 'Bus', 'Truck', 'Pedestrian', 'Cyclist', 'Tricycle', 'Vehicle']
    classes = oe.eval_classes(['Car', 'Bus', 'Truck', 'Pedestrian', 'Cyclist'], True)
    assert classes == ['Vehicle', 'Pedestrian', 'Cyclist']
    t = oe.accept_table(classes, names, True)
    assert t.tolist() == [[1, 1, 1, 0, 0, 1, 1], [0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0]]
    classes = oe.eval_classes(['Car', 'Bus', 'Truck', 'Pedestrian', 'Cyclist'], False)
    t = oe.accept_table(classes, names, False)
    assert t.tolist() == [[int(n == c) for n in names] for c in classes]
    assert oe.eval_classes(['Pedestrian', 'Cyclist'], True) == ['Vehicle', 'Pedestrian', 'Cyclist']
    with pytest.raises(AssertionError):
        oe.eval_classes(['Car', 'Pedestrian'], True)
    with pytest.raises(ValueError):
        oe._Plan(['Car'], names, False, None, 50, 'Hard')
    with pytest.raises(ValueError):
        oe._Plan(['Car'], names, False, {'Car': -0.5}, 50, 'Overall')


def test_fixture_covers_cases(golden):
    g = golden
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert g['gt_boxes'].dtype == np.float64 and g['pred_boxes'].dtype == np.float32
    names = [str(n) for n in g['names']]
    assert set(names) >= {'Car', 'Bus', 'Truck', 'Pedestrian', 'Cyclist'} and len(set(names) - set(g['classes'])) >= 1
    assert set(np.unique(g['pred_name'])) == set(range(len(names)))            # every name, the unknown one included
    assert 'Bus' not in {names[i] for i in g['gt_name']}                           # a class without GT
    assert (g['pred_count'] == 0).any() and (g['gt_count'] == 0).any()
    assert ((g['gt_count'] > 64) & (g['pred_count'] > 256)).any()
    po = np.concatenate([[0], np.cumsum(g['pred_count'])])
    ties = sum(len(s) - len(np.unique(s)) for s in np.split(g['pred_score'], po[1:-1]))
    assert ties > 0
    zeroed = (g['iou_heading'] == 0) & (g['iou_plain'] > 0.3)                      # flipped headings
    assert zeroed.sum() > 0
    thr = np.array([0.3, 0.5, 0.7])
    assert np.abs(g['iou_plain'][:, None] - thr).min() >= 1e-3
    for cfg in CONFIGS:
        assert cfg + '/counts' in g and str(g[cfg + '/ret_str']).startswith('\n|AP@')
    assert g['pr40/thresholds'].shape[1] == 41


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _frames(g, device='cuda'):
    from pdanet_amd import once_eval as oe
    gt, pred = _annos(g)
    vocab = oe._vocab([str(n) for n in g['names']])
    return oe.frames_from_annos(gt, pred, vocab, device), vocab


@pytest.mark.gpu
@pytest.mark.parametrize("heading", [True, False])
def test_iou_kernel_matches_reference(golden, heading):
    import torch
    from pdanet_amd import once_eval as oe, _lib
    fr, vocab = _frames(golden)
    iou = torch.full((fr.iou_total,), -7.0, dtype=torch.float64, device='cuda')
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    from pdanet_amd.pointnet2_batch_cuda import _call
    _call("pda_once_eval_iou", iou, ctypes.byref(fr.struct(fr.iou_start)), int(heading), iou.data_ptr(), status.data_ptr())
    got = iou.cpu().numpy()
    ref = golden['iou_heading' if heading else 'iou_plain']
    assert int(status.item()) == 0
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() < 2e-5
    if heading:
        flipped = (golden['iou_heading'] == 0) & (golden['iou_plain'] != 0)
        assert np.array_equal(got == 0, ref == 0) and (got[flipped] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_match_stage_on_reference_iou(golden, cfg):
    import torch
    from pdanet_amd import once_eval as oe
    kw = CONFIGS[cfg]
    fr, vocab = _frames(golden)
    plan = oe._Plan([str(c) for c in golden['classes']], list(vocab), kw.get('use_superclass', True), None,
                    kw.get('num_pr_points', 50), kw.get('difficulty_mode', 'Overall&Distance'))
    ref_iou = golden['iou_heading' if kw.get('ap_with_heading', True) else 'iou_plain']
    iou = torch.from_numpy(ref_iou).cuda()
    _, res = oe._run_stages(fr, plan, True, iou=iou)
    out = oe._read(res, plan)
    T = out['n_thresholds'].size
    nthr = out['n_thresholds'].reshape(T)
    assert np.array_equal(nthr, golden[cfg + '/n_thresholds'])
    assert np.array_equal(out['num_valid_gt'].reshape(T), golden[cfg + '/num_valid_gt'])
    thr = out['thresholds'].reshape(T, -1)
    counts = out['counts'].reshape(T, -1, 3)
    for t in range(T):
        n = nthr[t]
        assert np.array_equal(thr[t, :n].astype(np.float32), golden[cfg + '/thresholds'][t, :n].astype(np.float32))
        assert np.array_equal(counts[t, :n], golden[cfg + '/counts'][t, :n]), (cfg, t)


def _check_result(ret, golden, cfg):
    ret_str, ret_dict = ret
    assert list(ret_dict) == [str(k) for k in golden[cfg + '/keys']]
    np.testing.assert_allclose(np.array(list(ret_dict.values()), np.float64), golden[cfg + '/values'], rtol=0, atol=1e-9)
    assert ret_str == str(golden[cfg + '/ret_str'])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_end_to_end_from_annos(golden, cfg):
    from pdanet_amd import once_eval as oe
    gt, pred = _annos(golden)
    ret = oe.get_evaluation_results(gt, pred, [str(c) for c in golden['classes']], num_parts=7, **CONFIGS[cfg])
    _check_result(ret, golden, cfg)


def _padded_batches(pred, classes, batch, extra_cols=3):
    import torch
    out = []
    for s in range(0, len(pred), batch):
        chunk = pred[s:s + batch]
        K = max(1, max(len(p['name']) for p in chunk))
        boxes = torch.zeros(len(chunk), K, 7 + extra_cols)
        scores = torch.zeros(len(chunk), K)
        labels = torch.zeros(len(chunk), K, dtype=torch.int64)
        num = torch.zeros(len(chunk), dtype=torch.int32)
        for b, p in enumerate(chunk):
            n = len(p['name'])
            num[b] = n
            if n:
                boxes[b, :n, :7] = torch.from_numpy(np.asarray(p['boxes_3d'], np.float32))
                boxes[b, :n, 7:] = 0.5
                scores[b, :n] = torch.from_numpy(np.asarray(p['score'], np.float32))
                labels[b, :n] = torch.tensor([classes.index(str(x)) + 1 for x in p['name']])
        out.append({'pred_boxes': boxes.cuda(), 'pred_scores': scores.cuda(), 'pred_labels': labels.cuda(),
                    'num_pred': num.cuda()})
    return out


def _known_only(pred, classes):
    out = []
    for p in pred:
        keep = np.array([str(n) in classes for n in p['name']], bool)
        if keep.size and keep.any():
            out.append({'name': np.asarray(p['name'])[keep], 'score': np.asarray(p['score'])[keep],
                        'boxes_3d': np.asarray(p['boxes_3d'])[keep]})
        else:
            out.append({'name': np.zeros(0), 'score': np.zeros(0), 'boxes_3d': np.zeros((0, 7))})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ['default', 'no_superclass'])
def test_streaming_evaluator_matches_list_path(golden, cfg):
    from pdanet_amd import once_eval as oe
    classes = [str(c) for c in golden['classes']]
    gt, pred = _annos(golden)
    pred = _known_only(pred, classes)
    ref = oe.get_evaluation_results(gt, pred, classes, **CONFIGS[cfg])
    ev = oe.OnceEvaluator(classes, gt, **CONFIGS[cfg])
    for b in _padded_batches(pred, classes, 4):
        ev.add_batch(b)
    ret = ev.compute()
    assert ret[0] == ref[0] and list(ret[1]) == list(ref[1])
    assert all(ret[1][k] == ref[1][k] or (np.isnan(ret[1][k]) and np.isnan(ref[1][k])) for k in ref[1])


@pytest.mark.gpu
def test_add_batch_reads_nothing_back(golden):
    import torch
    from pdanet_amd import once_eval as oe
    classes = [str(c) for c in golden['classes']]
    gt, pred = _annos(golden)
    pred = _known_only(pred, classes)
    batches = _padded_batches(pred, classes, 8)
    ev = oe.OnceEvaluator(classes, gt)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for b in batches:
            ev.add_batch(b)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    ret = ev.compute()
    assert ret == oe.get_evaluation_results(gt, pred, classes)


# ---- validation-size sets ------------------------------------------------------------------------------------------------
_CLS = ['Car', 'Bus', 'Truck', 'Pedestrian', 'Cyclist']
_DIMS = np.array([(4.5, 1.9, 1.6), (11.0, 2.8, 3.2), (8.0, 2.6, 3.0), (0.7, 0.7, 1.7), (1.8, 0.8, 1.6)])


def _val_gt(rng, n_frames=3000, n_gt=40):
    """GT on a jittered 16 m grid (no two boxes overlap), no centre within 5 cm of the 30 / 50 m band edges."""
    gx, gy = np.meshgrid(np.arange(-72, 73, 16.0), np.arange(-72, 73, 16.0))
    cells = np.stack([gx.ravel(), gy.ravel()], 1)
    gts = []
    for _ in range(n_frames):
        while True:
            xy = cells[rng.choice(len(cells), n_gt, replace=False)] + rng.uniform(-2, 2, (n_gt, 2))
            z = rng.normal(0, 0.3, n_gt)
            d = np.sqrt(np.sum(np.c_[xy, z] ** 2, 1))
            if np.abs(d - 30).min() > 0.05 and np.abs(d - 50).min() > 0.05:
                break
        cls = rng.choice(5, n_gt, p=[0.5, 0.05, 0.1, 0.2, 0.15])
        dims = _DIMS[cls] * rng.uniform(0.9, 1.1, (n_gt, 3))
        boxes = np.c_[xy, z, dims, rng.uniform(-np.pi, np.pi, n_gt)]
        gts.append({'name': np.array(_CLS)[cls], 'boxes_3d': boxes})
    return gts


def _val_pred(rng, gts, max_pred=500):
    preds = []
    for g in gts:
        n = len(g['name'])
        hit = rng.random(n) < 0.8
        tb = g['boxes_3d'][hit] + np.c_[rng.normal(0, 0.2, (hit.sum(), 3)), np.zeros((hit.sum(), 4))]
        n_fp = int(rng.integers(50, max_pred - hit.sum()))
        fb = np.c_[rng.uniform(-75, 75, (n_fp, 2)), rng.normal(0, 0.5, n_fp), _DIMS[rng.integers(0, 5, n_fp)],
                   rng.uniform(-np.pi, np.pi, n_fp)]
        names = np.concatenate([g['name'][hit], np.array(_CLS)[rng.integers(0, 5, n_fp)]])
        scores = np.concatenate([rng.uniform(0.3, 1, hit.sum()), rng.uniform(0, 0.7, n_fp)]).astype(np.float32)
        preds.append({'name': names, 'score': scores, 'boxes_3d': np.concatenate([tb, fb]).astype(np.float32)})
    return preds


@pytest.fixture(scope="module")
def val_set():
    rng = np.random.default_rng(2024)
    gts = _val_gt(rng)
    return gts, _val_pred(rng, gts)


@pytest.mark.gpu
def test_val_size_frame_permutation_invariant(val_set):
    from pdanet_amd import once_eval as oe
    gts, preds = val_set
    ret = oe.get_evaluation_results(gts, preds, list(_CLS))
    perm = np.random.default_rng(5).permutation(len(gts))
    ret_p = oe.get_evaluation_results([gts[i] for i in perm], [preds[i] for i in perm], list(_CLS))
    assert ret_p[0] == ret[0] and ret_p[1] == ret[1]
    assert 0 < ret[1]['AP_mean/overall'] < 100


@pytest.mark.gpu
def test_val_size_perfect_and_empty_predictions(val_set):
    from pdanet_amd import once_eval as oe
    gts, _ = val_set
    shifted = [{'name': g['name'], 'score': np.ones(len(g['name']), np.float32),
                'boxes_3d': (g['boxes_3d'] + np.array([0.01, 0, 0, 0, 0, 0, 0])).astype(np.float32)} for g in gts]
    ret_str, ret = oe.get_evaluation_results(gts, shifted, list(_CLS))
    assert all(v == 100 for k, v in ret.items()), ret_str
    none = [{'name': np.zeros(0), 'score': np.zeros(0), 'boxes_3d': np.zeros((0, 7))} for _ in gts]
    ret_str, ret = oe.get_evaluation_results(gts, none, list(_CLS))
    assert all(v == 0 for v in ret.values()), ret_str
