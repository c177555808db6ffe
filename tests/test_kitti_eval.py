"""KITTI evaluation on the device (csrc/kitti_eval.hip, pdanet_amd/kitti_eval.py) against tests/golden/kitti_eval.npz,
which holds the reference's own eval.py / rotate_iou.py run on synthetic frames and its generate_prediction_dicts
geometry on synthetic calibrations (make_kitti_eval_golden.py)."""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "kitti_eval.npz")
CONFIGS = ('aos', 'no_aos')
# BEV / 3D: the stubbed reference runs numba's float64 promotions as numpy float32 scalar arithmetic (the fan area, the
# IoU denominators), so values differ by a few float32 steps
GEOM_TOL = 2e-5


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _annos(g, cfg):
    names = [str(n) for n in g['names']]
    go = np.concatenate([[0], np.cumsum(g['gt_count'])])
    do = np.concatenate([[0], np.cumsum(g['dt_count'])])
    gt, dt = [], []
    for f in range(len(g['gt_count'])):
        s = slice(go[f], go[f + 1])
        gt.append({'name': np.array([names[i] for i in g['gt_name'][s]], dtype='<U14'),
                   'truncated': g['gt_truncated'][s], 'occluded': g['gt_occluded'][s], 'alpha': g['gt_alpha'][s],
                   'bbox': g['gt_bbox'][s], 'dimensions': g['gt_dimensions'][s], 'location': g['gt_location'][s],
                   'rotation_y': g['gt_rotation_y'][s]})
        s = slice(do[f], do[f + 1])
        n = do[f + 1] - do[f]
        if n == 0:
            t = np.float64 if cfg == 'no_aos' else np.float32
            dt.append({'name': np.zeros(0), 'truncated': np.zeros(0), 'occluded': np.zeros(0), 'alpha': np.zeros(0, t),
                       'bbox': np.zeros([0, 4], t), 'dimensions': np.zeros([0, 3], t), 'location': np.zeros([0, 3], t),
                       'rotation_y': np.zeros(0, t), 'score': np.zeros(0, t)})
            continue
        alpha = g['dt_alpha'][s] if cfg == 'aos' else np.full(n, -10, np.float32)
        dt.append({'name': np.array([names[i] for i in g['dt_name'][s]]), 'truncated': np.zeros(n),
                   'occluded': np.zeros(n), 'alpha': alpha, 'bbox': g['dt_bbox'][s], 'dimensions': g['dt_dimensions'][s],
                   'location': g['dt_location'][s], 'rotation_y': g['dt_rotation_y'][s], 'score': g['dt_score'][s]})
    return gt, dt


@pytest.fixture(scope="module")
def lib():
    from pdanet_amd import build, _lib
    build.build()
    return _lib.load()


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_capi_argument_validation(lib):
    from pdanet_amd import _lib
    assert lib.pda_kitti_eval_workspace_bytes(-1, 10, 10, 3) == -1
    assert lib.pda_kitti_eval_workspace_bytes(3, 10, 10, 0) == -1
    assert lib.pda_kitti_eval_workspace_bytes(3, 10, 10, 7) == -1
    assert lib.pda_kitti_eval_workspace_bytes(3, 10, -1, 3) == -1
    assert lib.pda_kitti_eval_workspace_bytes(3, 10, 20, 3) >= 54 * 10 * 4 + 54 * 8 + 20 * 8 + 18 * 41 * 3 * 8
    st = lib.pda_kitti_eval_overlaps(None, None, None, None)
    assert st != 0 and b"null frames" in lib.pda_last_error()
    fr = _lib.KittiFrames(n_frames=2, max_gt=4, max_det=5000)
    st = lib.pda_kitti_eval_overlaps(ctypes.byref(fr), None, None, None)
    assert st != 0 and b"max_det" in lib.pda_last_error()
    fr = _lib.KittiFrames(n_frames=-1)
    assert lib.pda_kitti_eval_overlaps(ctypes.byref(fr), None, None, None) != 0
    fr = _lib.KittiFrames(n_frames=2, max_gt=4, max_det=8)               # frame arrays missing
    status = ctypes.c_int32(0)
    st = lib.pda_kitti_eval_overlaps(ctypes.byref(fr), None, ctypes.addressof(status), None)
    assert st != 0 and b"null frame arrays" in lib.pda_last_error()
    fr0 = _lib.KittiFrames(n_frames=0)
    gtc = (ctypes.c_int8 * 64 * 7)()
    dtc = (ctypes.c_uint8 * 64 * 7)()
    dc = (ctypes.c_uint8 * 64)()
    mo = (ctypes.c_double * 42)(*([0.5] * 42))
    args = lambda C, N: (ctypes.byref(fr0), None, C, N, gtc, dtc, dc, mo)
    for bad, msg in [((7, 4), b"n_classes"), ((0, 4), b"n_classes"), ((3, 65), b"n_names"), ((3, 0), b"n_names")]:
        assert lib.pda_kitti_eval_first_pass(*args(*bad), None, None, None, None, None, None) != 0
        assert msg in lib.pda_last_error()
        assert lib.pda_kitti_eval_match(*args(*bad), 1, *([None] * 11)) != 0
        assert msg in lib.pda_last_error()
    bad_mo = (ctypes.c_double * 18)(*([0.5] * 17 + [1.5]))
    assert lib.pda_kitti_eval_first_pass(ctypes.byref(fr0), None, 3, 4, gtc, dtc, dc, bad_mo, *([None] * 6)) != 0
    assert b"min_overlap" in lib.pda_last_error()
    gtc[0][2] = 5
    assert lib.pda_kitti_eval_first_pass(*args(3, 4), *([None] * 6)) != 0
    assert b"gt_class" in lib.pda_last_error()
    gtc[0][2] = 0
    assert lib.pda_kitti_eval_first_pass(*args(3, 4), *([None] * 6)) != 0
    assert b"null workspace" in lib.pda_last_error()
    assert lib.pda_kitti_eval_match(*args(3, 4), 1, *([None] * 11)) != 0
    assert b"null workspace" in lib.pda_last_error()
    for bad, msg in [((-1, 7, 1), b"n "), ((4, 6, 1), b"stride"), ((4, 7, 0), b"rows_per_frame")]:
        n, stride, rpf = bad
        assert lib.pda_kitti_eval_predictions(None, n, stride, rpf, None, None, None, 1, None, None, None,
                                              ctypes.addressof(status), None) != 0
        assert msg in lib.pda_last_error()
    assert lib.pda_kitti_eval_predictions(None, 4, 7, 1, None, None, None, 1, None, None, None, None, None) != 0
    assert b"null status" in lib.pda_last_error()


def test_class_tables_and_parts():
    from pdanet_amd import kitti_eval as ke
    assert ke.class_ids(['Car', 'Pedestrian', 2]) == [0, 1, 2] and ke.class_ids('Truck') == [5]
    with pytest.raises(KeyError):
        ke.class_ids(['Tram'])
    names = ['Car', 'VAN', 'person_sitting', 'Pedestrian', 'cyclist', 'DontCare', 'dontcare', 'Truck']
    gt, dt, dc = ke.name_tables([0, 1, 2, 5], names)
    assert gt.tolist() == [[1, 0, -1, -1, -1, -1, -1, -1], [-1, -1, 0, 1, -1, -1, -1, -1],
                           [-1, -1, -1, -1, 1, -1, -1, -1], [-1, -1, -1, -1, -1, -1, -1, 1]]
    assert dt.tolist() == (gt == 1).astype(np.uint8).tolist()
    assert dc.tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    assert ke.split_parts(30) == [30] and ke.split_parts(3769) == [37] * 100 + [69] and ke.split_parts(300) == [3] * 100
    f32 = {k: np.zeros((1, 4), np.float32) for k in ('bbox', 'location', 'dimensions')}
    f32.update({k: np.zeros(1, np.float32) for k in ('rotation_y', 'alpha', 'score')})
    f64 = {k: v.astype(np.float64) for k, v in f32.items()}
    gt = [{'bbox': np.zeros((1, 4), np.float32)}] * 4
    assert ke.frame_modes(gt, [f32] * 4, 2).tolist() == [0] * 4
    assert ke.frame_modes(gt, [f32, f32, f64, f32], 2).tolist() == [0, 0, 13, 13]           # GT bboxes stay float32
    gt64 = [{"bbox": np.zeros((1, 4))}] * 4
    assert ke.frame_modes(gt64, [f32] * 4, 2).tolist() == [2] * 4


def test_fixture_covers_cases(golden):
    g = golden
    assert os.path.getsize(GOLDEN) < 1 << 20
    names = [str(n) for n in g['names']]
    gt_names = {names[i] for i in g['gt_name']}
    assert gt_names >= {'Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'Misc', 'DontCare'}
    assert (g['gt_occluded'] >= 0).any() and set(np.unique(g['gt_occluded'][g['gt_occluded'] >= 0])) == {0, 1, 2, 3}
    for t in (0.15, 0.3, 0.5):
        assert (g['gt_truncated'] == t).any() and (np.abs(g['gt_truncated'] - t) < 0.02).sum() > (g['gt_truncated'] == t).sum()
    h = g['gt_bbox'][:, 3] - g['gt_bbox'][:, 1]
    assert ((h > 20) & (h < 30)).any() and ((h > 35) & (h < 45)).any() and np.abs(h[:, None] - [25, 40]).min() >= 1e-3
    dh = np.abs(g['dt_bbox'][:, 3] - g['dt_bbox'][:, 1])
    assert (dh < 25).any()
    assert (g['dt_count'] == 0).any() and (g['gt_count'] == 0).any()
    assert ((g['gt_count'] > 64) & (g['dt_count'] > 256)).any()
    do = np.concatenate([[0], np.cumsum(g['dt_count'])])
    assert sum(len(s) - len(np.unique(s)) for s in np.split(g['dt_score'], do[1:-1])) > 0
    C = len(g['classes'])
    assert (g['aos/num_valid_gt'].reshape(C, 3)[list(g['classes']).index('Truck')] == 0).all()
    ov = g['aos/overlaps']
    assert np.abs(ov.reshape(-1, 1) - np.array([0.25, 0.5, 0.7])).min() >= 1e-3
    assert ((ov[1] > 0.7) & (ov[2] > 0.7)).any()
    # DontCare suppression changes fp on metric 0
    assert 'aos/detail/aos' in g and 'no_aos/detail/aos' not in g
    assert 'aos  AP' in str(g['aos/result']) and 'aos  AP' not in str(g['no_aos/result'])


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _frames(g, cfg, device='cuda'):
    from pdanet_amd import kitti_eval as ke
    gt, dt = _annos(g, cfg)
    vocab = ke._vocab([str(n) for n in g['names']])
    return ke.frames_from_annos(gt, dt, vocab, device), vocab, gt, dt


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS)
def test_overlaps_match_reference(golden, cfg):
    import torch
    from pdanet_amd.pointnet2_batch_cuda import _call
    fr, _, _, _ = _frames(golden, cfg)
    ov = torch.full((3 * fr.ov_total,), -7.0, dtype=torch.float64, device='cuda')
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    _call("pda_kitti_eval_overlaps", ov, ctypes.byref(fr.struct()), ov.data_ptr(), status.data_ptr())
    got = ov.cpu().numpy().reshape(3, -1)
    ref = golden[cfg + '/overlaps']
    assert int(status.item()) == 0 and got.shape == ref.shape
    if cfg == 'aos':
        assert np.array_equal(got[0], ref[0])                               # all float32: exact
    else:
        # the float64 template of the empty frame makes the part's detection bboxes float64: numba unifies
        # min(float32, float64) to float64, the stub's Python min returns the float32 operand, a float32 step apart
        assert np.abs(got[0] - ref[0]).max() < 1e-6
        assert np.array_equal(got[0] > 0, ref[0] > 0)
    for m in (1, 2):
        assert np.abs(got[m] - ref[m]).max() < GEOM_TOL, m
        assert np.array_equal(got[m], got[m].astype(np.float32).astype(np.float64))   # stored as float32
        assert np.array_equal(got[m] > 0, ref[m] > 0)


def _plan(g):
    from pdanet_amd import kitti_eval as ke
    return ke._Plan([str(c) for c in g['classes']], [str(n) for n in g['names']])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS)
def test_statistics_on_reference_overlaps(golden, cfg):
    import torch
    from pdanet_amd import kitti_eval as ke
    fr, _, gt, dt = _frames(golden, cfg)
    plan = _plan(golden)
    aos = ke.compute_aos_of(dt)
    assert aos == (cfg == 'aos')
    ov = torch.from_numpy(np.ascontiguousarray(golden[cfg + '/overlaps']).reshape(-1)).cuda()
    _, (gtf, dtf), res = ke._run_stages(fr, plan, aos, overlaps=ov)
    out = ke._read(res, plan)
    C = plan.C
    assert np.array_equal(gtf.cpu().numpy().reshape(3 * C, -1), golden[cfg + '/gt_flags'])
    assert np.array_equal(dtf.cpu().numpy().reshape(3 * C, -1), golden[cfg + '/dt_flags'])
    assert np.array_equal(out['num_valid_gt'].reshape(-1), golden[cfg + '/num_valid_gt'])
    T = 18 * C
    nthr = out['n_thresholds'].reshape(T)
    assert np.array_equal(nthr, golden[cfg + '/n_thresholds'])
    thr = out['thresholds'].reshape(T, 41)
    counts = out['counts'].reshape(T, 41, 3)
    sim = out['similarity'].reshape(6 * C, 41)
    pr = golden[cfg + '/pr']
    for t in range(T):
        n = nthr[t]
        assert np.array_equal(thr[t, :n], golden[cfg + '/thresholds'][t, :n]), t
        assert np.array_equal(counts[t, :n], pr[t, :n, :3].astype(np.int64)), t
        if t < 6 * C:                                                        # metric 0
            ref = pr[t, :n, 3]
            assert np.all(np.abs(sim[t, :n] - ref) <= 1e-12 * np.abs(ref)), t
            if not aos:
                assert (sim[t] == 0).all()


def _check_result(ret, detail, golden, cfg, atol=1e-9):
    result, ret_dict = ret
    assert list(ret_dict) == [str(k) for k in golden[cfg + '/keys']]
    np.testing.assert_allclose(np.array([float(v) for v in ret_dict.values()]), golden[cfg + '/values'], rtol=0, atol=atol)
    assert result == str(golden[cfg + '/result'])
    keys = sorted(k.split('/', 2)[2] for k in golden if k.startswith(cfg + '/detail/'))
    assert sorted(detail) == keys
    for k in keys:
        np.testing.assert_allclose(detail[k], golden[cfg + '/detail/' + k], rtol=0, atol=atol, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS)
def test_end_to_end_from_annos(golden, cfg):
    from pdanet_amd import kitti_eval as ke
    gt, dt = _annos(golden, cfg)
    detail = {}
    ret = ke.get_official_eval_result(gt, dt, [str(c) for c in golden['classes']], PR_detail_dict=detail)
    _check_result(ret, detail, golden, cfg)


@pytest.mark.gpu
def test_two_runs_identical_bits(golden):
    from pdanet_amd import kitti_eval as ke
    fr, _, _, _ = _frames(golden, 'aos')
    plan = _plan(golden)
    a = ke._run_stages(fr, plan, True)[2].cpu().numpy()
    b = ke._run_stages(fr, plan, True)[2].cpu().numpy()
    assert np.array_equal(a, b)


@pytest.mark.gpu
def test_prediction_conversion_matches_reference(golden):
    import torch
    from pdanet_amd import kitti_eval as ke
    g = golden
    boxes = torch.from_numpy(g['pred/boxes']).cuda()
    fidx = torch.from_numpy(g['pred/frame']).cuda()
    calib = torch.from_numpy(g['pred/calib']).cuda()
    shape = torch.from_numpy(g['pred/image_shape']).cuda()
    cam, bbox, alpha, status = ke.convert_predictions(boxes, fidx, calib, shape)
    assert int(status.item()) == 0
    for got, ref in ((cam, g['pred/cam']), (bbox, g['pred/bbox']), (alpha, g['pred/alpha'])):
        got = got.cpu().numpy()
        ref = ref.astype(np.float32)
        assert got.dtype == np.float32 and got.shape == ref.shape
        # a few float32 steps of each value's magnitude (numpy's float32 matmul order is unspecified)
        assert np.all(np.abs(got - ref) <= 8 * np.spacing(np.maximum(np.abs(ref), 1).astype(np.float32)))
    # the dict form: one batch of frames, one of them empty
    calibs = [{'P2': c[:12].reshape(3, 4), 'R0': c[12:21].reshape(3, 3), 'Tr_velo2cam': c[21:].reshape(3, 4)}
              for c in g['pred/calib']]
    nf = len(calibs)
    preds = []
    for f in range(nf):
        sel = g['pred/frame'] == f
        n = int(sel.sum()) if f != 1 else 0
        preds.append({'pred_boxes': torch.from_numpy(g['pred/boxes'][sel][:n]).cuda(),
                      'pred_scores': torch.linspace(0.9, 0.1, n).cuda(),
                      'pred_labels': (torch.arange(n) % 3 + 1).cuda()})
    batch = {'frame_id': ['%06d' % f for f in range(nf)], 'calib': calibs,
             'image_shape': torch.from_numpy(g['pred/image_shape'])}
    annos = ke.generate_prediction_dicts(batch, preds, ['Car', 'Pedestrian', 'Cyclist'])
    keys = ['name', 'truncated', 'occluded', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score',
            'boxes_lidar', 'frame_id']
    for f, a in enumerate(annos):
        assert sorted(a) == sorted(keys) and a['frame_id'] == '%06d' % f
        sel = g['pred/frame'] == f
        if f == 1:
            assert a['bbox'].shape == (0, 4) and a['bbox'].dtype == np.float64 and a['name'].shape == (0,)
            continue
        n = int(sel.sum())
        assert a['name'].tolist() == [['Car', 'Pedestrian', 'Cyclist'][i % 3] for i in range(n)]
        assert a['bbox'].dtype == np.float32 and a['location'].dtype == np.float32
        tol = lambda r: 8 * np.spacing(np.maximum(np.abs(r), 1).astype(np.float32))
        for k, ref in (('bbox', g['pred/bbox'][sel]), ('location', g['pred/cam'][sel][:, :3]),
                       ('dimensions', g['pred/cam'][sel][:, 3:6]), ('rotation_y', g['pred/cam'][sel][:, 6]),
                       ('alpha', g['pred/alpha'][sel])):
            assert np.all(np.abs(a[k] - ref) <= tol(ref)), k
        assert np.array_equal(a['boxes_lidar'], g['pred/boxes'][sel])


def _padded(golden, frames):
    """post_processing-style padded tensors of the golden detections, via their lidar boxes: the camera boxes are
    converted back through a calibration of identity R0 and the axis-swap V2C, so the device conversion recovers them."""
    import torch
    g = golden
    names = [str(n) for n in g['names']]
    classes = [str(c) for c in g['classes']]
    do = np.concatenate([[0], np.cumsum(g['dt_count'])])
    out = []
    P2 = np.array([[720, 0, 621, 0], [0, 720, 187, 0], [0, 0, 1, 0]], np.float32)
    V2C = np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0]], np.float32)
    calib_row = np.concatenate([P2.reshape(-1), np.eye(3, dtype=np.float32).reshape(-1), V2C.reshape(-1)])
    for s in range(0, len(frames), 4):
        chunk = frames[s:s + 4]
        K = max(1, max(do[f + 1] - do[f] for f in chunk))
        boxes = torch.zeros(len(chunk), K, 9)
        scores = torch.zeros(len(chunk), K)
        labels = torch.zeros(len(chunk), K, dtype=torch.int64)
        num = torch.zeros(len(chunk), dtype=torch.int32)
        for b, f in enumerate(chunk):
            sl = slice(do[f], do[f + 1])
            keep = np.array([names[i] in classes for i in g['dt_name'][sl]], bool)
            n = int(keep.sum())
            num[b] = n
            if n:
                loc, dims, ry = g['dt_location'][sl][keep], g['dt_dimensions'][sl][keep], g['dt_rotation_y'][sl][keep]
                # camera (x, y, z, l, h, w, ry) -> lidar (z, -x, -y + h / 2, l, w, h, -ry - pi / 2)
                lid = np.stack([loc[:, 2], -loc[:, 0], -loc[:, 1] + dims[:, 1] / 2, dims[:, 0], dims[:, 2], dims[:, 1],
                                -ry - np.float32(np.pi / 2)], 1).astype(np.float32)
                boxes[b, :n, :7] = torch.from_numpy(lid)
                scores[b, :n] = torch.from_numpy(g['dt_score'][sl][keep])
                labels[b, :n] = torch.tensor([classes.index(names[i]) + 1 for i in g['dt_name'][sl][keep]])
        out.append(({'pred_boxes': boxes.cuda(), 'pred_scores': scores.cuda(), 'pred_labels': labels.cuda(),
                     'num_pred': num.cuda()},
                    torch.from_numpy(np.tile(calib_row, (len(chunk), 1))).cuda(),
                    torch.tensor([[375, 1242]] * len(chunk), dtype=torch.int32).cuda()))
    return out


def _as_list(golden, batches, classes):
    """What generate_prediction_dicts makes of the same padded batches: the list path's input."""
    from pdanet_amd import kitti_eval as ke
    annos = []
    for padded, calib, shape in batches:
        B = padded['num_pred'].shape[0]
        preds = [{'pred_boxes': padded['pred_boxes'][b, :int(padded['num_pred'][b])],
                  'pred_scores': padded['pred_scores'][b, :int(padded['num_pred'][b])],
                  'pred_labels': padded['pred_labels'][b, :int(padded['num_pred'][b])]} for b in range(B)]
        c = calib.cpu().numpy()
        calibs = [{'P2': r[:12].reshape(3, 4), 'R0': r[12:21].reshape(3, 3), 'Tr_velo2cam': r[21:].reshape(3, 4)} for r in c]
        annos += ke.generate_prediction_dicts({'frame_id': list(range(B)), 'calib': calibs, 'image_shape': shape.cpu()},
                                              preds, classes)
    return annos


@pytest.mark.gpu
def test_streaming_evaluator_matches_list_path(golden):
    from pdanet_amd import kitti_eval as ke
    classes = [str(c) for c in golden['classes']]
    gt, _ = _annos(golden, 'aos')
    batches = _padded(golden, list(range(len(gt))))
    dt = _as_list(golden, batches, classes)
    d_ref, d_got = {}, {}
    ref = ke.get_official_eval_result(gt, dt, classes, PR_detail_dict=d_ref)
    ev = ke.KittiEvaluator(classes, gt)
    for padded, calib, shape in batches:
        ev.add_batch(padded, calib, shape)
    ret = ev.compute(PR_detail_dict=d_got)
    assert ret[0] == ref[0] and list(ret[1]) == list(ref[1])
    assert all(ret[1][k] == ref[1][k] or (np.isnan(ret[1][k]) and np.isnan(ref[1][k])) for k in ref[1])
    assert sorted(d_got) == sorted(d_ref) and all(np.array_equal(d_got[k], d_ref[k], equal_nan=True) for k in d_ref)
    assert 'aos  AP' in ret[0]


@pytest.mark.gpu
def test_add_batch_reads_nothing_back(golden):
    import torch
    from pdanet_amd import kitti_eval as ke
    classes = [str(c) for c in golden['classes']]
    gt, _ = _annos(golden, 'aos')
    batches = _padded(golden, list(range(len(gt))))
    ev = ke.KittiEvaluator(classes, gt)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for padded, calib, shape in batches:
            ev.add_batch(padded, calib, shape)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    ret = ev.compute()
    assert ret == ke.get_official_eval_result(gt, _as_list(golden, batches, classes), classes)


# ---- KITTI-val-sized sets ------------------------------------------------------------------------------------------------
_CLS = ['Car', 'Pedestrian', 'Cyclist']
_DIMS = np.array([(3.9, 1.55, 1.6), (0.8, 1.75, 0.6), (1.75, 1.7, 0.6)])


def _val_gt(rng, n_frames=3769, n_gt=12):
    """GT on a jittered 6 m grid in front of the camera (no two boxes overlap), bbox heights away from 25 / 40."""
    gx, gz = np.meshgrid(np.arange(-24, 25, 6.0), np.arange(8, 60, 6.0))
    cells = np.stack([gx.ravel(), gz.ravel()], 1)
    gts = []
    for _ in range(n_frames):
        cls = rng.choice(3, n_gt, p=[0.6, 0.25, 0.15])
        xz = cells[rng.choice(len(cells), n_gt, replace=False)] + rng.uniform(-1, 1, (n_gt, 2))
        dims = _DIMS[cls] * rng.uniform(0.9, 1.1, (n_gt, 3))
        loc = np.c_[xz[:, 0], rng.uniform(1.5, 1.8, n_gt), xz[:, 1]].astype(np.float32)
        top = rng.uniform(100, 200, n_gt)
        h = rng.choice([12.0, 30.0, 60.0], n_gt) + rng.uniform(-3, 3, n_gt)
        x0 = rng.uniform(0, 1100, n_gt)
        bbox = np.c_[x0, top, x0 + rng.uniform(20, 120, n_gt), top + h].astype(np.float32)
        gts.append({'name': np.array(_CLS)[cls], 'truncated': rng.choice([0.0, 0.2, 0.4, 0.8], n_gt),
                    'occluded': rng.integers(0, 4, n_gt).astype(np.float64), 'alpha': rng.uniform(-np.pi, np.pi, n_gt),
                    'bbox': bbox, 'dimensions': dims, 'location': loc, 'rotation_y': rng.uniform(-np.pi, np.pi, n_gt)})
    return gts


def _val_dt(rng, gts, n_fp=20):
    dts = []
    for g in gts:
        n = len(g['name'])
        hit = rng.random(n) < 0.8
        m = int(hit.sum())
        loc = np.concatenate([g['location'][hit] + rng.normal(0, 0.1, (m, 3)),
                              np.c_[rng.uniform(-25, 25, n_fp), np.full(n_fp, 1.6), rng.uniform(8, 60, n_fp)]])
        dims = np.concatenate([g['dimensions'][hit], _DIMS[rng.integers(0, 3, n_fp)]])
        ry = np.concatenate([g['rotation_y'][hit] + rng.normal(0, 0.1, m), rng.uniform(-np.pi, np.pi, n_fp)])
        x0 = rng.uniform(0, 1100, n_fp)
        bbox = np.concatenate([g['bbox'][hit] + rng.normal(0, 2, (m, 4)),
                               np.c_[x0, np.full(n_fp, 150.0), x0 + 50, np.full(n_fp, 150.0) + rng.uniform(10, 60, n_fp)]])
        names = np.concatenate([g['name'][hit], np.array(_CLS)[rng.integers(0, 3, n_fp)]])
        dts.append({'name': names, 'alpha': np.concatenate([g['alpha'][hit], rng.uniform(-3, 3, n_fp)]).astype(np.float32),
                    'bbox': bbox.astype(np.float32), 'dimensions': dims.astype(np.float32),
                    'location': loc.astype(np.float32), 'rotation_y': ry.astype(np.float32),
                    'score': np.concatenate([rng.uniform(0.3, 1, m), rng.uniform(0, 0.7, n_fp)]).astype(np.float32)})
    return dts


@pytest.fixture(scope="module")
def val_set():
    rng = np.random.default_rng(2024)
    gts = _val_gt(rng)
    return gts, _val_dt(rng, gts)


@pytest.mark.gpu
def test_val_size_frame_permutation_invariant(val_set):
    from pdanet_amd import kitti_eval as ke
    gts, dts = val_set
    ret = ke.get_official_eval_result(gts, dts, _CLS)
    perm = np.random.default_rng(5).permutation(len(gts))
    ret_p = ke.get_official_eval_result([gts[i] for i in perm], [dts[i] for i in perm], _CLS)
    assert ret_p[0] == ret[0]
    assert all(abs(ret_p[1][k] - ret[1][k]) <= 1e-9 for k in ret[1])       # AOS sums in another frame order
    assert all(0 < v < 100 for k, v in ret[1].items() if 'image' in k), ret[0]


@pytest.mark.gpu
def test_val_size_perfect_and_empty_predictions(val_set):
    from pdanet_amd import kitti_eval as ke
    gts, _ = val_set
    # 5 cm off in x and z and turned by 0.02 rad: coincident or nearly collinear edges are degenerate for the reference's
    # float32 intersection (identical rectangles give 0), so "perfect" boxes are close, not equal
    perfect = [{'name': g['name'], 'alpha': g['alpha'].astype(np.float32), 'bbox': g['bbox'],
                'dimensions': g['dimensions'].astype(np.float32),
                'location': g['location'] + np.array([0.05, 0, 0.05], np.float32),
                'rotation_y': (g['rotation_y'] + 0.02).astype(np.float32), 'score': np.ones(len(g['name']), np.float32)}
               for g in gts]
    result, ret = ke.get_official_eval_result(gts, perfect, _CLS)
    # AOS: float32 detection alphas against float64 GT alphas leave (1 + cos(delta)) / 2 a few 1e-16 under 1
    assert all(abs(v - 100) < 1e-9 for v in ret.values()), result
    assert all(v == 100 for k, v in ret.items() if '_aos/' not in k), result
    none = [{'name': np.zeros(0), 'alpha': np.zeros(0), 'bbox': np.zeros((0, 4)), 'dimensions': np.zeros((0, 3)),
             'location': np.zeros((0, 3)), 'rotation_y': np.zeros(0), 'score': np.zeros(0)} for _ in gts]
    result, ret = ke.get_official_eval_result(gts, none, _CLS)
    assert all(v == 0 for v in ret.values()), result
