"""3-D recall of the eval loop on the device (csrc/recall.hip, model_nms_utils.recall_record / RecallRecorder, the detector's
eval return) against tests/golden/recall.npz, which holds the reference's own generate_recall_record run per scene as its
post_processing runs it (make_recall_golden.py)."""
import ctypes
import os
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "recall.npz")
THRESH = [0.3, 0.5, 0.7]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _batches(g):
    out = []
    for i in range(int(g['n_batches'])):
        p = 'b%d_' % i
        rec = dict(zip([str(k) for k in g[p + 'recall_keys']], [int(v) for v in g[p + 'recall_vals']]))
        out.append(dict(case=str(g[p + 'case']), pred=g[p + 'pred'], num=g[p + 'num'], gt=g.get(p + 'gt'),
                        thresh=[float(t) for t in g[p + 'thresh']], recall=rec, max_iou=g[p + 'max_iou']))
    return out


def _kept(gt_scene):
    k = gt_scene.shape[0] - 1
    while k > 0 and gt_scene[k].sum(dtype=np.float32) == 0:
        k -= 1
    return k + 1 if gt_scene.shape[0] else 0


@pytest.fixture(scope="module")
def lib():
    from pdanet_amd import build, _lib
    build.build()
    return _lib.load()


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_capi_argument_validation(lib):
    thr = (ctypes.c_float * 16)(*([0.5] * 16))
    call = lambda gt_cols, n_thresh, b, k, t: lib.pda_recall_record(None, None, None, gt_cols, thr, n_thresh, None, None,
                                                                     b, k, t, None)
    for args, word in [((8, 3, -1, 10, 4), b"b=-1"), ((8, 3, 2, -1, 4), b"k=-1"), ((8, 3, 2, 10, -1), b"t=-1"),
                       ((8, -1, 2, 10, 4), b"n_thresh=-1"), ((8, 17, 2, 10, 4), b"n_thresh=17"),
                       ((6, 3, 2, 10, 4), b"gt_cols=6"), ((8, 3, 70000, 10, 4), b"batch"),
                       ((8, 3, 2, 10, 4), b"null pointer")]:
        assert call(*args) == 1, args
        assert word in lib.pda_last_error(), (args, lib.pda_last_error())
    assert call(8, 3, 0, 10, 4) == 0 and call(8, 16, 2, 10, 0) == 0          # nothing to count, no launch


def test_fixture_covers_cases(golden):
    bs = _batches(golden)
    cases = [b['case'] for b in bs]
    for c in ("kitti16", "kitti64", "once", "exact", "thresh", "trim", "no_pred", "max_gt0", "no_gt"):
        assert c in cases, c
    kitti = [b for b in bs if b['case'].startswith('kitti')]
    assert {b['gt'].shape[1] for b in kitti} == {16, 64} and all(b['pred'].shape[0] == 4 for b in kitti)
    once = [b for b in bs if b['case'] == 'once']
    assert all(b['pred'].shape[0] == 2 for b in once) and max(int(b['num'].max()) for b in once) == 500
    real = np.concatenate([b['max_iou'][np.isfinite(b['max_iou'])] for b in kitti + once])
    for lo, hi in [(0.1, 0.3), (0.3, 0.5), (0.5, 0.7), (0.7, 0.95)]:
        assert ((real > lo) & (real <= hi)).sum() >= 5, (lo, hi)
    assert (real == 0).sum() >= 5                                            # GT without any overlapping prediction
    # false positives, duplicates, headings next to +-pi
    assert sum(int(b['num'].sum()) for b in kitti) > 2 * sum(int(np.isfinite(b['max_iou']).sum()) for b in kitti)
    heads = np.concatenate([b['gt'][..., 6].ravel() for b in kitti] + [b['pred'][..., 6].ravel() for b in kitti])
    assert (np.abs(np.abs(heads) - np.pi) < 2e-4).sum() >= 5
    # touching boxes and boxes 1e-4 apart (axis-aligned, same y, x gap 0 / 1e-4)
    gaps = []
    for b in kitti + once:
        for s in range(b['pred'].shape[0]):
            p, g = b['pred'][s, :b['num'][s]], b['gt'][s]
            for q in p[(p[:, 6] == 0)]:
                m = (g[:, 6] == 0) & (g[:, 1] == q[1]) & (g[:, 3] > 0)
                gaps += list(np.abs(q[0] - g[m, 0]) - (q[3] + g[m, 3]) / 2)
    gaps = np.array(gaps)
    assert (np.abs(gaps) < 1e-5).any() and (np.abs(gaps - 1e-4) < 2e-5).any()
    ex = next(b for b in bs if b['case'] == 'exact')
    assert (ex['max_iou'] == 0.5).sum() == 2 and (ex['max_iou'] > 0.99).sum() == 2
    assert ex['recall']['rcnn_0.5'] == ex['recall']['rcnn_0.3'] - 2          # IoU exactly 0.5 is not > 0.5
    th = next(b for b in bs if b['case'] == 'thresh')
    t32 = np.array(th['thresh'], np.float32)
    assert len(th['thresh']) <= 16 and len(set(t32.tolist())) < len(th['thresh'])
    for t in th['thresh']:                                                   # a float64 comparison would count more
        m = th['max_iou'][np.isfinite(th['max_iou'])].astype(np.float64)
        if float(np.float32(t)) > t and t < 0.99:
            assert (m > t).sum() > th['recall']['rcnn_%s' % t]
    tr = next(b for b in bs if b['case'] == 'trim')
    g = tr['gt']
    assert (g[0, 2] == 0).all() and np.isfinite(tr['max_iou'][0, 2])          # zero row in the middle: kept
    assert (g[1] == 0).all() and np.isfinite(tr['max_iou'][1, 0]) and np.isnan(tr['max_iou'][1, 1:]).all()
    assert g[2, 5].any() and g[2, 5].sum(dtype=np.float32) == 0 and np.isnan(tr['max_iou'][2, 5])
    assert tr['num'][3] == 0 and (tr['max_iou'][3] == 0).all()
    assert tr['recall']['gt'] == sum(_kept(g[s]) for s in range(g.shape[0])) == 5 + 1 + 5 + 8
    npd = next(b for b in bs if b['case'] == 'no_pred')
    assert (npd['num'] == 0).all() and npd['recall']['gt'] > 0 and npd['recall']['rcnn_0.3'] == 0
    assert next(b for b in bs if b['case'] == 'max_gt0')['recall']['gt'] == 0
    nog = next(b for b in bs if b['case'] == 'no_gt')
    assert nog['gt'] is None and nog['recall'] == {}
    assert os.path.getsize(GOLDEN) < 500 * 1024


def test_from_config_and_compute_without_gpu():
    import torch
    from pdanet_amd import config
    from pdanet_amd.model_nms_utils import RecallRecorder, recall_dict, recall_record
    for name in ("kitti_pda_ssd.yaml", "once_pda_ssd.yaml"):
        pp = config.load_yaml(name)["MODEL"]["POST_PROCESSING"]
        rec = RecallRecorder.from_config(pp, device='cpu')
        assert rec.enabled and rec.thresh_list == THRESH and rec.counters.tolist() == [0, 0, 0, 0]
    assert not RecallRecorder.from_config({'RECALL_MODE': 'speed', 'RECALL_THRESH_LIST': [0.5]}, device='cpu').enabled
    assert RecallRecorder.from_config({'RECALL_THRESH_LIST': [0.25]}, device='cpu').enabled      # reference default
    rec = RecallRecorder([0.3, 0.5], device='cpu')
    assert rec.compute() == ({'gt_num': 0, 'recall_roi_0.3': 0, 'recall_rcnn_0.3': 0, 'recall_roi_0.5': 0,
                              'recall_rcnn_0.5': 0},
                             {'recall/roi_0.3': 0.0, 'recall/rcnn_0.3': 0.0, 'recall/roi_0.5': 0.0, 'recall/rcnn_0.5': 0.0})
    rec.counters += torch.tensor([8, 6, 2])
    metric, ret = rec.compute()
    assert metric['gt_num'] == 8 and metric['recall_rcnn_0.3'] == 6 and ret['recall/rcnn_0.5'] == 0.25
    assert list(recall_dict([5, 3, 1], [0.3, 0.5])) == ['gt', 'roi_0.3', 'rcnn_0.3', 'roi_0.5', 'rcnn_0.5']
    with pytest.raises(ValueError):
        RecallRecorder([0.1] * 17, device='cpu')
    with pytest.raises(TypeError):                                          # device float32 only
        recall_record(torch.zeros(1, 4, 7), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 3, 8), THRESH)


# ---- GPU -----------------------------------------------------------------------------------------------------------------
def _dev(b):
    import torch
    gt = None if b['gt'] is None else torch.from_numpy(b['gt']).cuda()
    return torch.from_numpy(b['pred']).cuda(), torch.from_numpy(b['num']).cuda(), gt


def _run(b, lib=None):
    import torch
    from pdanet_amd.model_nms_utils import recall_record
    pred, num, gt = _dev(b)
    mi = torch.full((pred.shape[0], gt.shape[1]), float('nan'), device='cuda')
    cnt = recall_record(pred, num, gt, b['thresh'], max_iou=mi)
    return cnt.cpu().numpy(), mi.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.gpu
def test_max_iou_bit_identical_to_boxes_iou3d_and_fixture(golden):
    import torch
    from pdanet_amd import iou3d_nms_utils as iu
    for b in _batches(golden):
        if b['gt'] is None:
            continue
        _, mi = _run(b)
        assert np.array_equal(_bits(mi), _bits(b['max_iou'])), b['case']
        pred, _, gt = _dev(b)
        for s in range(pred.shape[0]):
            n, kept = int(b['num'][s]), _kept(b['gt'][s])
            if n and kept:
                want = iu.boxes_iou3d_gpu(pred[s, :n], gt[s, :kept, :7].contiguous()).max(0)[0].cpu().numpy()
                assert np.array_equal(_bits(mi[s, :kept]), _bits(want)), (b['case'], s)


@pytest.mark.gpu
def test_counters_equal_reference_recall_dicts(golden):
    from pdanet_amd.model_nms_utils import recall_dict
    for b in _batches(golden):
        if b['gt'] is None:
            continue
        cnt, _ = _run(b)
        assert recall_dict(cnt.tolist(), b['thresh']) == b['recall'], b['case']


def _reference_recall(preds, gt, thresh):
    """generate_recall_record's loop on this repository's boxes_iou3d_gpu (host reads as the reference makes them)."""
    from pdanet_amd import iou3d_nms_utils as iu
    ret = {}
    for s, p in enumerate(preds):
        if not ret:
            ret = {'gt': 0}
            for t in thresh:
                ret['roi_%s' % str(t)] = 0
                ret['rcnn_%s' % str(t)] = 0
        cur = gt[s]
        k = cur.__len__() - 1
        while k > 0 and cur[k].sum() == 0:
            k -= 1
        cur = cur[:k + 1]
        if cur.shape[0] > 0:
            box = p['pred_boxes']
            iou = iu.boxes_iou3d_gpu(box[:, 0:7].contiguous(), cur[:, 0:7].contiguous()) if box.shape[0] > 0 else None
            for t in thresh:
                if iou is not None:
                    ret['rcnn_%s' % str(t)] += (iou.max(dim=0)[0] > t).sum().item()
            ret['gt'] += cur.shape[0]
    return ret


def _kitti_batch():
    import torch
    from pdanet_amd import data_processor, detector
    torch.manual_seed(7)
    model, cfg = detector.build_detector("kitti_pda_ssd.yaml")
    model = model.cuda().eval()
    rng = np.random.default_rng(44)
    scenes, boxes = [], []
    for n, m in ((20000, 9), (16000, 14)):
        p = np.zeros((n, 4), np.float32)
        p[:, 0], p[:, 1], p[:, 2], p[:, 3] = rng.uniform(2, 68, n), rng.uniform(-38, 38, n), rng.uniform(-2.5, 0.5, n), \
            rng.uniform(0, 1, n)
        b = np.zeros((m, 8), np.float32)
        b[:, 0], b[:, 1], b[:, 2] = rng.uniform(5, 65, m), rng.uniform(-35, 35, m), -1.0
        b[:, 3:6] = [3.9, 1.6, 1.5]
        b[:, 6], b[:, 7] = rng.uniform(-np.pi, np.pi, m), rng.integers(1, 4, m)
        scenes.append(p)
        boxes.append(b)
    dp = data_processor.from_config(cfg, training=False)
    bd = dp(scenes, boxes, max_gt=32, seed=9)
    return model, cfg, bd


def _count_syncs(fn):
    import torch
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    return out, sum("called a synchronizing" in str(x.message) for x in w)     # not the once-only "prototype" notice


@pytest.mark.gpu
def test_kitti_detector_eval_returns_reference_recall():
    import torch
    from pdanet_amd import model_nms_utils
    model, cfg, bd = _kitti_batch()
    assert bd['gt_boxes'].shape == (2, 32, 8)
    pp = model.model_cfg["POST_PROCESSING"]
    assert pp["RECALL_MODE"] == "normal"
    with torch.no_grad():
        try:
            for mode in ("normal", "speed"):              # first calls: one-time setup reads back
                pp["RECALL_MODE"] = mode
                model(dict(bd))
            pp["RECALL_MODE"] = "normal"
            (preds, rec), n_normal = _count_syncs(lambda: model(dict(bd)))
            pp["RECALL_MODE"] = "speed"
            (preds_s, rec_s), n_speed = _count_syncs(lambda: model(dict(bd)))
        finally:
            pp["RECALL_MODE"] = "normal"
    assert rec_s == {}
    assert n_normal == n_speed >= 1, (n_normal, n_speed)
    assert rec == _reference_recall(preds, bd['gt_boxes'], THRESH) and rec['gt'] == int(bd['input_info'][:, 2].sum())
    assert set(rec) == {'gt', 'roi_0.3', 'rcnn_0.3', 'roi_0.5', 'rcnn_0.5', 'roi_0.7', 'rcnn_0.7'}
    assert all(isinstance(v, int) for v in rec.values())
    for a, b in zip(preds, preds_s):
        for k in ('pred_boxes', 'pred_scores', 'pred_labels'):
            assert torch.equal(a[k], b[k]), k
    # the same batch_dict through post_processing in both modes: every key but 'recall' is bit-identical
    with torch.no_grad():
        model(bd)
    p_n = model_nms_utils.post_processing(bd, dict(pp, RECALL_MODE='normal'), model.num_class)
    p_s = model_nms_utils.post_processing(bd, dict(pp, RECALL_MODE='speed'), model.num_class)
    assert set(p_n) == set(p_s) | {'recall'}
    assert all(torch.equal(p_n[k], p_s[k]) for k in p_s)
    no_gt = {k: v for k, v in bd.items() if k != 'gt_boxes'}
    with torch.no_grad():
        preds_n, rec_n = model(no_gt)
    assert rec_n == {} and len(preds_n) == 2


@pytest.mark.gpu
def test_recorder_add_reads_nothing_and_replays_in_a_graph(golden):
    import torch
    from pdanet_amd.model_nms_utils import RecallRecorder
    b = next(x for x in _batches(golden) if x['case'] == 'kitti64')
    pred, num, gt = _dev(b)
    padded = {'pred_boxes': pred, 'num_pred': num}
    rec = RecallRecorder(b['thresh'])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rec.add(padded, gt)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    eager = rec.counters.clone()
    assert eager.tolist() == list(b['recall'].values())[0:1] + [b['recall']['rcnn_%s' % t] for t in b['thresh']]
    rec.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rec.add(padded, gt)
    rec.reset()
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(rec.counters, eager * 5)


@pytest.mark.gpu
def test_streaming_equals_sum_of_batches(golden):
    import torch
    from pdanet_amd.model_nms_utils import RecallRecorder
    bs = [b for b in _batches(golden) if b['thresh'] == THRESH]
    rec = RecallRecorder(THRESH)
    total = {}
    for b in bs:
        pred, num, gt = _dev(b)
        rec.add({'pred_boxes': pred, 'num_pred': num}, gt)
        for k, v in b['recall'].items():
            total[k] = total.get(k, 0) + v
    metric, ret = rec.compute()
    assert metric == {'gt_num': total['gt'], **{('recall_' + k): total[k] for k in total if k != 'gt'}}
    for t in THRESH:
        assert ret['recall/rcnn_%s' % t] == total['rcnn_%s' % t] / max(total['gt'], 1)
        assert ret['recall/roi_%s' % t] == 0.0
    empty = RecallRecorder(THRESH)
    b0 = next(b for b in bs if b['case'] == 'max_gt0')
    pred, num, gt = _dev(b0)
    empty.add({'pred_boxes': pred, 'num_pred': num}, gt)
    empty.add({'pred_boxes': pred, 'num_pred': num}, None)
    metric, ret = empty.compute()
    assert metric['gt_num'] == 0 and all(v == 0.0 for v in ret.values()) and len(ret) == 6


@pytest.mark.gpu
def test_two_runs_identical_bits(golden):
    for b in _batches(golden):
        if b['gt'] is None:
            continue
        c1, m1 = _run(b)
        c2, m2 = _run(b)
        assert np.array_equal(c1, c2) and np.array_equal(_bits(m1), _bits(m2)), b['case']


# ---- KITTI-val-sized set -----------------------------------------------------------------------------------------------
def _val_set(rng, n_frames=3769, max_gt=64):
    n_gt = rng.integers(1, max_gt + 1, n_frames)
    gt = np.zeros((n_frames, max_gt, 8), np.float32)
    for f in range(n_frames):
        m = n_gt[f]
        gx, gy = np.meshgrid(np.arange(0, 70, 8.0), np.arange(-36, 37, 8.0))
        cells = np.stack([gx.ravel(), gy.ravel()], 1)[rng.choice(90, m, replace=False)]
        gt[f, :m, 0:2] = cells + rng.uniform(-1, 1, (m, 2))
        gt[f, :m, 2] = rng.uniform(-1.8, -0.6, m)
        gt[f, :m, 3:6] = np.array([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.2, (m, 3))
        gt[f, :m, 6] = rng.uniform(-np.pi, np.pi, m)
        gt[f, :m, 7] = rng.integers(1, 4, m)
    return gt, n_gt


@pytest.fixture(scope="module")
def val_set():
    return _val_set(np.random.default_rng(3769))


def _val_recall(gt, preds, nums, batch=4):
    import torch
    from pdanet_amd.model_nms_utils import RecallRecorder
    rec = RecallRecorder(THRESH)
    gt_d, p_d, n_d = torch.from_numpy(gt).cuda(), torch.from_numpy(preds).cuda(), torch.from_numpy(nums).cuda()
    for s in range(0, gt.shape[0], batch):
        rec.add({'pred_boxes': p_d[s:s + batch], 'num_pred': n_d[s:s + batch]}, gt_d[s:s + batch])
    return rec.compute()


@pytest.mark.gpu
def test_val_size_perfect_empty_and_permuted(val_set):
    gt, n_gt = val_set
    metric, ret = _val_recall(gt, np.ascontiguousarray(gt[..., :7]), n_gt.astype(np.int32))
    assert metric['gt_num'] == int(n_gt.sum())
    assert all(ret['recall/rcnn_%s' % t] == 1.0 for t in THRESH), ret
    metric0, ret0 = _val_recall(gt, np.zeros((gt.shape[0], 50, 7), np.float32), np.zeros(gt.shape[0], np.int32))
    assert metric0['gt_num'] == int(n_gt.sum()) and all(v == 0.0 for v in ret0.values())
    # jittered predictions plus false positives, 50 a frame; the same rows in another order inside each frame
    rng = np.random.default_rng(7)
    preds = np.zeros((gt.shape[0], 50, 7), np.float32)
    nums = np.zeros(gt.shape[0], np.int32)
    for f in range(gt.shape[0]):
        hit = np.nonzero(rng.random(n_gt[f]) < 0.7)[0][:40]
        p = gt[f, hit, :7] + rng.normal(0, 0.25, (len(hit), 7)).astype(np.float32) * [1, 1, 0.2, 0.2, 0.1, 0.1, 0.2]
        fp = np.c_[rng.uniform(0, 70, (10, 1)), rng.uniform(-40, 40, (10, 1)), np.full((10, 1), -1.0),
                   np.tile([3.9, 1.6, 1.56], (10, 1)), rng.uniform(-3, 3, (10, 1))]
        p = np.concatenate([p, fp]).astype(np.float32)
        preds[f, :len(p)], nums[f] = p, len(p)
    metric1, ret1 = _val_recall(gt, preds, nums)
    perm = preds.copy()
    for f in range(gt.shape[0]):
        perm[f, :nums[f]] = preds[f, rng.permutation(nums[f])]
    metric2, ret2 = _val_recall(gt, perm, nums)
    assert metric1 == metric2 and ret1 == ret2
    assert 0 < ret1['recall/rcnn_0.7'] < ret1['recall/rcnn_0.5'] < ret1['recall/rcnn_0.3'] < 1
