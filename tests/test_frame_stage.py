"""Preparing frames on the device (pdanet_amd/frame_stage.py, csrc/frame_stage.hip): KITTI's field-of-view filter and the
gt_sampling database, against the reference's outputs recorded in tests/golden/frame_stage.npz
(tests/golden/make_frame_stage_golden.py) and against numpy restatements that live here.

The float32 restatement of the FOV expression (fov_restatement) runs op by op in float32, as the kernel does.  The
reference forms the same sums with a float32 matrix product whose order of operations is BLAS's, so its flags are compared
outside a band a float64 evaluation draws: 1e-2 px around the four image limits, 1e-3 m around depth 0."""
import ctypes
import importlib.util
import os
import pickle

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "frame_stage.npz")
i64 = ctypes.c_int64
BAND_PX, BAND_M, BAND_SHARE = 1e-2, 1e-3, 1e-3


def _golden():
    return dict(np.load(GOLDEN))


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, *path))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _rows(a, off):
    return [a[off[b]:off[b + 1]] for b in range(len(off) - 1)]


# ---- numpy restatements ------------------------------------------------------------------------------------------------------
def calib_records_np(P2, R0, V2C):
    """M | P2 (24 float32): M = np.dot(V2C.T, R0.T) in float32, as Calibration.lidar_to_rect forms it."""
    P2, R0, V2C = (np.asarray(a, np.float32) for a in (P2, R0, V2C))
    return np.concatenate([np.dot(V2C.T, R0.T).reshape(12), P2.reshape(12)]).astype(np.float32)


def fov_restatement(pts, rec, shape):
    """get_fov_flag behind lidar_to_rect / rect_to_img, every operation a separately rounded float32 one."""
    x, y, z = (np.ascontiguousarray(pts[:, k], np.float32) for k in range(3))
    M, P = np.asarray(rec[:12], np.float32).reshape(4, 3), np.asarray(rec[12:], np.float32).reshape(3, 4)
    with np.errstate(all="ignore"):
        r = [((x * M[0, k] + y * M[1, k]) + z * M[2, k]) + M[3, k] for k in range(3)]
        h = [((r[0] * P[j, 0] + r[1] * P[j, 1]) + r[2] * P[j, 2]) + P[j, 3] for j in range(3)]
        assert all(a.dtype == np.float32 for a in r + h)
        u, v, depth = h[0] / r[2], h[1] / r[2], h[2] - P[2, 3]
        H, W = int(shape[0]), int(shape[1])
        return (u >= 0) & (u < W) & (v >= 0) & (v < H) & (depth >= 0)


def fov_float64(pts, P2, R0, V2C, shape):
    P2, R0, V2C = (np.asarray(a, np.float64) for a in (P2, R0, V2C))
    hom = np.concatenate([pts[:, :3].astype(np.float64), np.ones((len(pts), 1))], 1)
    rect = hom @ (V2C.T @ R0.T)
    h = np.concatenate([rect, np.ones((len(pts), 1))], 1) @ P2.T
    with np.errstate(all="ignore"):
        u, v, depth = h[:, 0] / rect[:, 2], h[:, 1] / rect[:, 2], h[:, 2] - P2[2, 3]
        H, W = int(shape[0]), int(shape[1])
        return (u >= 0) & (u < W) & (v >= 0) & (v < H) & (depth >= 0), u, v, depth


def fov_band(pts, P2, R0, V2C, shape):
    """Points a float64 evaluation puts within 1e-2 px of an image limit or 1e-3 m of depth 0: either answer is accepted."""
    _, u, v, depth = fov_float64(pts, P2, R0, V2C, shape)
    H, W = int(shape[0]), int(shape[1])
    with np.errstate(all="ignore"):
        near = (np.abs(u) <= BAND_PX) | (np.abs(u - W) <= BAND_PX) | (np.abs(v) <= BAND_PX) | (np.abs(v - H) <= BAND_PX)
        return near | (np.abs(depth) <= BAND_M) | ~np.isfinite(u) | ~np.isfinite(v)


def points_in_boxes_np(points, boxes):
    return _load("make_augment_golden", "golden", "make_augment_golden.py").points_in_boxes_cpu_np(points, boxes)


def extract_np(points, boxes64):
    """create_groundtruth_database's loop body: per box the points inside, shifted by the float64 centre in place."""
    masks = points_in_boxes_np(points[:, :3], np.asarray(boxes64, np.float32))
    out = []
    for i in range(len(boxes64)):
        p = points[masks[i] > 0].copy()
        p[:, :3] -= np.asarray(boxes64, np.float64)[i, :3]
        out.append(p)
    return out


def _kitti_scenes(g):
    P = _rows(g["kitti_points"], g["kitti_offsets"])
    cid = g["kitti_calib_id"]
    return P, cid, [g["image_shapes"][c] for c in cid]


def _calib_rows(g):
    """(n_calibs, 33) rows P2 | R0 | V2C, the public calibration form (kitti_eval.calib_matrix)."""
    return np.concatenate([g["calib_P2"].reshape(-1, 12), g["calib_R0"].reshape(-1, 9), g["calib_V2C"].reshape(-1, 12)], 1).astype(np.float32)


def _kitti_frames(g):
    bo = g["kitti_box_offsets"]
    P = _rows(g["kitti_points"], g["kitti_offsets"])
    return P, _rows(g["kitti_boxes"], bo), [list(x) for x in _rows(g["kitti_names"], bo)], [str(x) for x in g["kitti_frame_ids"]], \
        {k: _rows(g["kitti_" + k], bo) for k in ("difficulty", "bbox", "score")}


def _assert_infos_equal(mine, ref, keys):
    assert list(mine) == list(ref)                                   # classes in order of first appearance
    for name in ref:
        assert len(mine[name]) == len(ref[name]), name
        for a, b in zip(mine[name], ref[name]):
            assert tuple(a) == keys and tuple(b) == keys             # the reference's keys, in its order
            for k in keys:
                if k in ("box3d_lidar", "bbox"):
                    assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.array_equal(a[k], b[k]), (name, k)
                else:
                    assert a[k] == b[k], (name, k)


# ---- without a GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pdanet_amd import build, _lib
    build.build()
    return _lib.load()


def test_fixture_covers_the_cases():
    g = _golden()
    P, cid, shapes = _kitti_scenes(g)
    sizes = [len(p) for p in P]
    assert sum(20000 <= n <= 30000 for n in sizes) >= 3
    for p in [p for p in P if len(p) >= 20000]:                      # the full circle
        ang = np.arctan2(p[:, 1], p[:, 0])
        assert np.histogram(ang, bins=12, range=(-np.pi, np.pi))[0].min() > 500
    assert len(g["calib_P2"]) == 2 and {tuple(s) for s in g["image_shapes"]} == {(375, 1242), (370, 1224)}
    flags = _rows(g["kitti_fov_flag"], g["kitti_offsets"])
    assert any(f.sum() == 0 and len(f) > 0 for f in flags)           # a scene with no point in view
    assert any(n == 0 for n in np.diff(g["kitti_box_offsets"]))      # a scene with no boxes
    assert len(g["once_points"]) > 0 and len(g["once_boxes"]) > 0
    assert os.path.getsize(GOLDEN) < 1500000


def test_restatement_equals_the_reference_flags():
    g = _golden()
    P, cid, shapes = _kitti_scenes(g)
    flags = _rows(g["kitti_fov_flag"], g["kitti_offsets"])
    for b, p in enumerate(P):
        c = cid[b]
        rec = calib_records_np(g["calib_P2"][c], g["calib_R0"][c], g["calib_V2C"][c])
        assert np.array_equal(rec[:12].reshape(4, 3), g["calib_M"][c])                   # M as the reference formed it
        mine = fov_restatement(p, rec, shapes[b])
        band = fov_band(p, g["calib_P2"][c], g["calib_R0"][c], g["calib_V2C"][c], shapes[b])
        print("scene %d: %d points, %d kept, %d in the band, %d differ" % (b, len(p), flags[b].sum(), band.sum(), (mine != flags[b]).sum()))
        assert band.mean() <= BAND_SHARE, b
        assert np.array_equal(mine[~band], flags[b][~band]), b
    for b, (s, e) in enumerate(g["kitti_edge_ranges"]):              # the near-edge points: outside the band, so exact
        c = cid[b]
        rec = calib_records_np(g["calib_P2"][c], g["calib_R0"][c], g["calib_V2C"][c])
        p = P[b][s:e]
        assert e - s >= 100
        assert not fov_band(p, g["calib_P2"][c], g["calib_R0"][c], g["calib_V2C"][c], shapes[b]).any()
        _, u, v, depth = fov_float64(p, g["calib_P2"][c], g["calib_R0"][c], g["calib_V2C"][c], shapes[b])
        H, W = shapes[b]
        edge = np.minimum.reduce([np.abs(u), np.abs(u - W), np.abs(v), np.abs(v - H)])
        assert ((edge > 0.04) & (edge < 0.51)).sum() >= 90 and (np.abs(np.abs(depth) - 0.01) < 1e-3).sum() >= 10
        kept = fov_restatement(p, rec, shapes[b])
        assert np.array_equal(kept, flags[b][s:e]) and kept.any() and not kept.all()


def test_calib_records_follow_the_public_form():
    from pdanet_amd import frame_stage as fs
    g = _golden()
    rec = fs.calib_records(_calib_rows(g))
    for c in range(2):
        assert np.array_equal(rec[c], calib_records_np(g["calib_P2"][c], g["calib_R0"][c], g["calib_V2C"][c]))
    dicts = [{"P2": g["calib_P2"][c], "R0": g["calib_R0"][c], "Tr_velo2cam": g["calib_V2C"][c]} for c in range(2)]
    assert np.array_equal(fs.calib_records(dicts), rec)


def test_new_entries_validate_their_arguments(lib):
    assert lib.pda_abi_version() == 20
    assert lib.pda_kitti_fov_filter_workspace_bytes(4, i64(120000)) > 0
    assert lib.pda_kitti_fov_filter_workspace_bytes(-1, i64(1000)) == -1
    assert lib.pda_kitti_fov_filter_workspace_bytes(2, i64(0)) == -1
    assert lib.pda_gt_extract_workspace_bytes(4, i64(120000), i64(160)) >= 160 * 469 * 4
    assert lib.pda_gt_extract_workspace_bytes(4, i64(120000), i64(0)) == 0
    assert lib.pda_gt_extract_workspace_bytes(4, i64(120000), i64(-1)) == -1
    assert lib.pda_gt_extract_workspace_bytes(4, i64(0), i64(8)) == -1

    def fov(batch=2, c=4, n_cap=10, n_total=0, out_cap=0):
        return lib.pda_kitti_fov_filter(None, None, i64(n_total), batch, c, i64(n_cap), None, None, None, i64(out_cap), None, None,
                                        None, None)

    def count(batch=2, c=4, n_cap=10, n_total=0, m_total=0):
        return lib.pda_gt_extract_count(None, None, i64(n_total), batch, c, i64(n_cap), None, None, i64(m_total), None, None, None,
                                        None)

    def write(batch=2, c=4, n_cap=10, n_total=0, m_total=3, out_cap=0):
        return lib.pda_gt_extract_write(None, None, i64(n_total), batch, c, i64(n_cap), None, None, i64(m_total), None, None, None,
                                        i64(out_cap), None, None, None)

    for fn, name in ((fov, b"pda_kitti_fov_filter"), (count, b"pda_gt_extract_count"), (write, b"pda_gt_extract_write")):
        assert fn(batch=0) == 0                                                          # an empty problem
        assert fn(c=2) == 1 and b"bad size" in lib.pda_last_error() and name in lib.pda_last_error()
        assert fn(c=65) == 1 and b"bad size" in lib.pda_last_error()
        assert fn(n_cap=0) == 1 and b"bad size" in lib.pda_last_error()
        assert fn(n_total=-1) == 1 and b"bad size" in lib.pda_last_error()
        assert fn(batch=-1) == 1 and b"bad size" in lib.pda_last_error()
        assert fn() == 1 and b"null" in lib.pda_last_error() and name in lib.pda_last_error()   # sizes fine, no buffers
    assert fov(out_cap=-1) == 1 and b"bad size" in lib.pda_last_error()
    assert count(m_total=-1) == 1 and b"bad size" in lib.pda_last_error()
    assert write(out_cap=-1) == 1 and b"bad size" in lib.pda_last_error()
    assert write(m_total=0) == 0                                                         # no boxes: nothing to write


def test_camera_to_lidar_equals_the_reference():
    from pdanet_amd import box_utils
    g = _golden()
    for c in range(2):
        calib = {"P2": g["calib_P2"][c], "R0": g["calib_R0"][c], "Tr_velo2cam": g["calib_V2C"][c]}
        for tag in ("f32", "f64"):
            cam = g["cam_boxes_" + tag].copy()
            out = box_utils.boxes3d_kitti_camera_to_lidar(cam, calib)
            ref = g["lidar_boxes_%s_%d" % (tag, c)]
            assert out.dtype == ref.dtype and np.array_equal(out, ref), (c, tag)
            assert np.array_equal(cam, g["cam_boxes_" + tag])                            # the input is left alone


@pytest.mark.parametrize("dataset", ["kitti", "once"])
def test_dbinfos_writer_from_recorded_counts(dataset):
    """The info dictionaries and file names from the fixture's recorded counts: no device involved."""
    from pdanet_amd import frame_stage as fs
    g = _golden()
    ref = pickle.loads(g[dataset + "_dbinfos"].tobytes())
    counts = np.diff(g[dataset + "_db_point_offsets"])
    if dataset == "kitti":
        P, B, N, ids, extra = _kitti_frames(g)
        builder = fs.GtDatabaseBuilder(used_classes=[str(x) for x in g["kitti_used_classes"]])
        bo = g["kitti_box_offsets"]
        for f in range(len(ids)):
            builder.add_counted(ids[f], N[f], B[f], counts[bo[f]:bo[f + 1]], {k: v[f] for k, v in extra.items()})
        keys = fs.KITTI_KEYS
        assert any(o["name"] not in builder.used_classes for o in builder.objects)       # the used_classes rule is exercised
    else:
        builder = fs.GtDatabaseBuilder()
        builder.add_counted(str(g["once_frame_id"]), list(g["once_names"]), g["once_boxes"], counts)
        keys = fs.ONCE_KEYS
    assert [builder.file_name(o) for o in builder.objects] == [str(x) for x in g[dataset + "_db_files"]]
    _assert_infos_equal(builder.dbinfos(dataset, "train"), ref, keys)
    assert builder.dbinfos(dataset, "val")[next(iter(ref))][0]["path"].startswith("gt_database_val/")


def test_extract_restatement_equals_the_recorded_bins():
    g = _golden()
    P, B, N, ids, extra = _kitti_frames(g)
    got = [o for f in range(len(ids)) for o in extract_np(P[f], B[f])]
    ref = _rows(g["kitti_db_points"], g["kitti_db_point_offsets"])
    assert len(got) == len(ref) and all(np.array_equal(a, b) for a, b in zip(got, ref))


# ---- GPU: the FOV filter -------------------------------------------------------------------------------------------------------
def _unpack(res):
    (pts, offs, n_cap), info = res
    o = offs.cpu().numpy()
    p = pts.cpu().numpy()
    return [p[o[b]:o[b + 1]] for b in range(len(o) - 1)], o, info.cpu().numpy()


def _assert_fov(res, scenes, recs, shapes):
    out, o, info = _unpack(res)
    assert o[0] == 0
    for b, p in enumerate(scenes):
        keep = fov_restatement(p, recs[b], shapes[b])
        print("scene %d: %d points, %d kept (device %d)" % (b, len(p), keep.sum(), len(out[b])))
        assert info[b].tolist() == [len(p), int(keep.sum()), 0, 0], b
        assert o[b + 1] - o[b] == keep.sum()
        assert np.array_equal(out[b].view(np.uint32), p[keep].view(np.uint32)), b        # kept set, order and bits


@pytest.mark.gpu
def test_fov_filter_equals_the_restatement_on_the_fixture():
    from pdanet_amd import frame_stage as fs
    g = _golden()
    P, cid, shapes = _kitti_scenes(g)
    rows = _calib_rows(g)[cid]
    recs = [calib_records_np(g["calib_P2"][c], g["calib_R0"][c], g["calib_V2C"][c]) for c in cid]
    res = fs.fov_filter(P, rows, np.array(shapes))
    _assert_fov(res, P, recs, shapes)
    flags = _rows(g["kitti_fov_flag"], g["kitti_offsets"])
    out, _, info = _unpack(res)
    for b, (s, e) in enumerate(g["kitti_edge_ranges"]):              # near-edge points: exactly the reference's set
        assert np.array_equal(out[b][-int(flags[b][s:e].sum()):], P[b][s:e][flags[b][s:e]])
    assert info[3, 1] == 0 and info[3, 0] > 0                        # the scene with no point in view
    # other feature counts take the scalar path; NaN coordinates keep nothing
    for C in (3, 5):
        Q = [np.concatenate([p[:, :3], np.tile(p[:, 3:4], (1, C - 3))], 1) if C > 3 else p[:, :3].copy() for p in P[:2]]
        Q[0][5, 0] = np.nan
        Q[0][6, 2] = np.inf
        _assert_fov(fs.fov_filter(Q, rows[:2], np.array(shapes[:2])), Q, recs[:2], shapes[:2])


def _random_scans(rng, B, n, C=4):
    ang, r = rng.uniform(-np.pi, np.pi, (B, n)), rng.uniform(1.0, 80.0, (B, n))
    p = np.zeros((B, n, C), np.float32)
    p[..., 0], p[..., 1] = r * np.cos(ang), r * np.sin(ang)
    p[..., 2] = rng.uniform(-3.0, 2.0, (B, n))
    p[..., 3:] = rng.uniform(0, 1, (B, n, C - 3))
    return p


@pytest.mark.gpu
def test_fov_filter_equals_the_restatement_on_a_random_batch():
    from pdanet_amd import frame_stage as fs
    g = _golden()
    rng = np.random.default_rng(11)
    p = _random_scans(rng, 4, 120000)
    scenes = [p[0], p[1][:100003], p[2], p[3][:77]]
    cid = [0, 1, 1, 0]
    shapes = [g["image_shapes"][c] for c in cid]
    recs = [calib_records_np(g["calib_P2"][c], g["calib_R0"][c], g["calib_V2C"][c]) for c in cid]
    _assert_fov(fs.fov_filter(scenes, _calib_rows(g)[cid], np.array(shapes)), scenes, recs, shapes)


@pytest.mark.gpu
def test_fov_filter_reads_nothing_back_and_flags_bad_scenes():
    from pdanet_amd import frame_stage as fs
    g = _golden()
    rng = np.random.default_rng(12)
    p = _random_scans(rng, 2, 30000)
    packed = torch.from_numpy(p.reshape(-1, 4)).cuda()
    offs = torch.tensor([0, 30000, 60000], dtype=torch.int64, device="cuda")
    cal = torch.from_numpy(fs.calib_records(_calib_rows(g))).cuda()
    shp = torch.from_numpy(g["image_shapes"].astype(np.int32)).cuda()
    ref = fs.fov_filter((packed, offs, 30000), cal, shp)                                 # loads the kernels
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = fs.fov_filter((packed, offs, 30000), cal, shp, check=False)
        host = fs.fov_filter((packed, offs, 30000), _calib_rows(g), g["image_shapes"], check=False)   # host calibs: one async copy
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    for res in (out, host):
        assert torch.equal(res[0][1], ref[0][1]) and torch.equal(res[1], ref[1])
        n = int(ref[0][1][-1])
        assert n > 0 and torch.equal(res[0][0][:n], ref[0][0][:n])
    # a scene over n_cap and a scene whose offsets leave the buffer are written empty and flagged
    bad = torch.tensor([0, 30000, 70000], dtype=torch.int64, device="cuda")
    (pts, o, _), info = fs.fov_filter((packed, bad, 30000), cal, shp, check=False)
    assert info.cpu()[:, 3].tolist() == [0, fs.STATUS_BAD_OFFSETS] and o.cpu().tolist() == [0, int(ref[1][0, 1]), int(ref[1][0, 1])]
    (pts, o, _), info = fs.fov_filter((packed, offs, 29999), cal, shp, check=False)
    assert info.cpu().tolist() == [[0, 0, 0, fs.STATUS_OVER_CAP]] * 2 and o.cpu().tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        fs.fov_filter((packed, offs, 29999), cal, shp)


@pytest.mark.gpu
def test_fov_filter_feeds_the_data_processor():
    from pdanet_amd import frame_stage as fs, data_processor as dpm
    g = _golden()
    P, cid, shapes = _kitti_scenes(g)
    sel = [0, 1, 2]
    scenes = [P[b] for b in sel]
    recs = [calib_records_np(g["calib_P2"][cid[b]], g["calib_R0"][cid[b]], g["calib_V2C"][cid[b]]) for b in sel]
    host = [p[fov_restatement(p, r, shapes[b])] for p, r, b in zip(scenes, recs, sel)]
    k = 4096
    cfg = [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
           {"NAME": "sample_points", "NUM_POINTS": {"train": k, "test": k}},
           {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": True, "test": False}}]
    dp = dpm.DataProcessor(cfg, [0.0, -40.0, -3.0, 70.4, 40.0, 1.0], True, 4)
    rng = np.random.default_rng(5)
    draws = {"pick": [rng.integers(0, 1000, k) for _ in sel], "perm1": [rng.permutation(k) for _ in sel],
             "perm2": [rng.permutation(k) for _ in sel]}
    dev_tuple, _ = fs.fov_filter(scenes, _calib_rows(g)[cid[sel]], np.array([shapes[b] for b in sel]))
    a = dp(dev_tuple, draws=draws)
    b = dp(host, draws=draws)
    assert torch.equal(a["points"], b["points"]) and torch.equal(a["input_info"], b["input_info"])
    assert (a["input_info"][:, 3] == 0).all() and a["points"].shape == (3 * k, 5)


# ---- GPU: the database -----------------------------------------------------------------------------------------------------------
def _kitti_builder(g):
    from pdanet_amd import frame_stage as fs
    P, B, N, ids, extra = _kitti_frames(g)
    builder = fs.GtDatabaseBuilder(used_classes=[str(x) for x in g["kitti_used_classes"]])
    builder.add_frames(P[:2], B[:2], N[:2], ids[:2], {k: v[:2] for k, v in extra.items()})         # two batches
    builder.add_frames(P[2:], B[2:], N[2:], ids[2:], {k: v[2:] for k, v in extra.items()})
    return builder


def _once_builder(g):
    from pdanet_amd import frame_stage as fs
    builder = fs.GtDatabaseBuilder()
    builder.add_frames([g["once_points"]], [g["once_boxes"]], [list(g["once_names"])], [str(g["once_frame_id"])])
    return builder


@pytest.mark.gpu
@pytest.mark.parametrize("dataset", ["kitti", "once"])
def test_database_equals_the_reference(dataset, tmp_path):
    from pdanet_amd import frame_stage as fs
    g = _golden()
    builder = _kitti_builder(g) if dataset == "kitti" else _once_builder(g)
    path = builder.write(str(tmp_path), dataset=dataset, split="train")
    assert os.path.basename(path) == dataset + "_dbinfos_train.pkl"
    files = [str(x) for x in g[dataset + "_db_files"]]
    assert sorted(os.listdir(tmp_path / "gt_database")) == sorted(files)
    ref_bins = _rows(g[dataset + "_db_points"], g[dataset + "_db_point_offsets"])
    in_two = 0
    for name, ref in zip(files, ref_bins):
        with open(tmp_path / "gt_database" / name, "rb") as f:
            assert f.read() == ref.tobytes(), name                                       # byte-identical
    with open(path, "rb") as f:
        mine = pickle.load(f)
    ref = pickle.loads(g[dataset + "_dbinfos"].tobytes())
    _assert_infos_equal(mine, ref, fs.KITTI_KEYS if dataset == "kitti" else fs.ONCE_KEYS)
    if dataset == "kitti":
        assert "Van" not in mine and any(n.split("_")[1] == "Van" for n in files)        # a .bin for every object, infos for used_classes
        P, B, N, ids, extra = _kitti_frames(g)
        in_two = (points_in_boxes_np(P[1][:, :3], B[1]).sum(0) >= 2).sum()
        assert in_two >= 5                                                               # points in two overlapping boxes


@pytest.mark.gpu
def test_written_database_reads_back_as_the_built_one(tmp_path):
    from pdanet_amd import data_augmentor as da
    g = _golden()
    builder = _kitti_builder(g)
    builder.write(str(tmp_path), dataset="kitti", split="train")
    names = [str(x) for x in g["kitti_used_classes"]]
    for prepare in ({}, {"filter_by_min_points": ["Car:60", "Pedestrian:5", "Cyclist:90"], "filter_by_difficulty": [-1]}):
        cfg = {"DB_INFO_PATH": ["kitti_dbinfos_train.pkl"], "NUM_POINT_FEATURES": 4, "PREPARE": prepare}
        a = da.GtDatabase.from_dbinfos(str(tmp_path), cfg, names, device="cuda")
        b = builder.finish(names, cfg)
        assert a.n_obj == b.n_obj and a.n_obj > 0 and a.num_point_features == b.num_point_features
        for key in ("points", "offsets", "boxes", "centre", "classes"):
            x, y = getattr(a, key), getattr(b, key)
            assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), key
        assert np.array_equal(a.sizes, b.sizes) and np.array_equal(a.host_boxes, b.host_boxes)
        assert a.start == b.start and a.count == b.count
    full = da.GtDatabase.from_dbinfos(str(tmp_path), {"DB_INFO_PATH": ["kitti_dbinfos_train.pkl"], "NUM_POINT_FEATURES": 4}, names, device="cuda")
    assert a.n_obj < full.n_obj                                                          # the filters removed something


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["once", "kitti"])
def test_augmentor_with_a_built_database_reproduces_the_augment_fixture(tag, tmp_path):
    """tests/golden/augment.npz's case with its database rebuilt through the builder.  The fixture stores every object
    cloud relative to a float64 centre that is no float32 number, so no float32 frame would give the cloud back bit for
    bit; each cloud is therefore extracted in its object's own frame (the box at the origin: every point is inside and
    the shift is exact) and the builder's records then get the fixture's box3d_lidar.  What is shown is that the device
    construction (extract -> finish -> from_device) and from_dbinfos are interchangeable."""
    from pdanet_amd import data_augmentor as da, frame_stage as fs
    ta = _load("test_augment", "test_augment.py")
    ga = ta._golden()
    names, cfg, infos, bins, scenes = ta._case(ga, tag)
    builder = fs.GtDatabaseBuilder()
    objs = [i for name in infos for i in infos[name]]
    frames, boxes = [], []
    for i in objs:
        box = np.array(i["box3d_lidar"], np.float64)
        box[:3] = 0.0
        frames.append(bins[i["path"]])
        boxes.append(box[None])
    extra = {"difficulty": [[i["difficulty"]] for i in objs]}
    for s in range(0, len(objs), 16):
        builder.add_frames(frames[s:s + 16], boxes[s:s + 16], [[i["name"]] for i in objs[s:s + 16]],
                           ["%06d" % k for k in range(s, min(s + 16, len(objs)))], {"difficulty": extra["difficulty"][s:s + 16]})
    assert [o["num_points_in_gt"] for o in builder.objects] == [i["num_points_in_gt"] for i in objs]
    for o, i in zip(builder.objects, objs):
        o["box3d_lidar"] = i["box3d_lidar"]
    sampler_cfg = cfg["AUG_CONFIG_LIST"][0]
    db = builder.finish(names, sampler_cfg)
    ta._write_db(str(tmp_path), infos, bins)
    ref_db = da.GtDatabase.from_dbinfos(str(tmp_path), sampler_cfg, names, device="cuda")
    for key in ("points", "offsets", "boxes", "centre", "classes"):
        assert torch.equal(getattr(db, key), getattr(ref_db, key)), key
    assert db.start == ref_db.start and db.count == ref_db.count and np.array_equal(db.sizes, ref_db.sizes)
    planes, calib = ta._road(ga, tag)
    outs = []
    for database in (db, ref_db):
        aug = da.DataAugmentor(cfg, names, database)
        pt, bt, info = aug([s[0] for s in scenes], [s[1] for s in scenes], [da.class_ids(s[2], names) for s in scenes],
                           plan=ta._plan(ga, tag), road_planes=planes, calib=calib)
        outs.append(ta._unpack(pt, bt, info))
    refP = ta._rows(ga, tag + "_ref_points", tag + "_ref_offsets")
    refB = ta._rows(ga, tag + "_ref_boxes", tag + "_ref_box_offsets")
    for b in range(len(scenes)):
        assert np.array_equal(outs[0][0][b], outs[1][0][b]) and np.array_equal(outs[0][1][b], outs[1][1][b])
        assert outs[0][0][b].shape == refP[b].shape and outs[0][1][b].shape == refB[b].shape
        assert np.array_equal(outs[0][0][b][:, 3:], refP[b][:, 3:]) and np.array_equal(outs[0][1][b][:, 7], refB[b][:, 7])
        assert ta._ulps(outs[0][0][b][:, :3], refP[b][:, :3]).max() <= 4 and ta._ulps(outs[0][1][b][:, :7], refB[b][:, :7]).max() <= 4
    assert np.array_equal(outs[0][2], outs[1][2])


def _near_face64(points, boxes, tol):
    """Points a float64 evaluation puts within tol of a face of a box (x / y limits carry the margin (double)1e-2f)."""
    bad = np.zeros(len(points), bool)
    m = float(np.float32(1e-2))
    p = points.astype(np.float64)
    for b in np.asarray(boxes, np.float32).astype(np.float64):
        c, s = np.cos(-b[6]), np.sin(-b[6])
        sx, sy = p[:, 0] - b[0], p[:, 1] - b[1]
        lx, ly = sx * c - sy * s, sx * s + sy * c
        for v, h in ((lx, b[3] / 2 + m), (ly, b[4] / 2 + m), (p[:, 2] - b[2], b[5] / 2)):
            bad |= np.abs(np.abs(v) - h) < tol
    return bad


@pytest.mark.gpu
def test_extraction_of_a_large_random_batch():
    from pdanet_amd import frame_stage as fs
    rng = np.random.default_rng(21)
    B, n, m = 4, 120000, 40
    scans = _random_scans(rng, B, n)
    frames, boxes = [], []
    for b in range(B):
        bx = np.concatenate([rng.uniform(-60, 60, (m, 2)), rng.uniform(-1.5, 0.5, (m, 1)), rng.uniform(1.5, 12.0, (m, 2)),
                             rng.uniform(1.5, 4.0, (m, 1)), rng.uniform(-np.pi, np.pi, (m, 1))], 1)
        bx[:, :3] = bx[:, :3].astype(np.float32)
        p = scans[b][~_near_face64(scans[b], bx, 1e-5)]
        frames.append(p)
        boxes.append(bx)
    from pdanet_amd import stage_common
    packed, offs_h, n_cap, _ = stage_common.pack_scenes(frames)
    allb = np.concatenate(boxes)
    dev = "cuda"
    obj_points, obj_offs, counts, info = fs.gt_extract(
        (torch.from_numpy(packed).to(dev), torch.from_numpy(offs_h).to(dev), n_cap), torch.from_numpy(allb.astype(np.float32)).to(dev),
        torch.arange(0, B * m + 1, m, dtype=torch.int64, device=dev), torch.from_numpy(np.ascontiguousarray(allb[:, :3])).to(dev))
    exp = [o for b in range(B) for o in extract_np(frames[b], boxes[b])]
    print("extracted %d rows into %d objects, largest %d" % (sum(len(e) for e in exp), len(exp), max(len(e) for e in exp)))
    assert counts.cpu().tolist() == [len(e) for e in exp] and sum(len(e) for e in exp) > 10000
    assert info.cpu().tolist() == [[len(frames[b]), m, 0, 0] for b in range(B)]
    got = _rows(obj_points.cpu().numpy(), obj_offs.cpu().numpy())
    for k, (a, e) in enumerate(zip(got, exp)):
        assert np.array_equal(a.view(np.uint32), e.view(np.uint32)), k


@pytest.mark.gpu
def test_a_frame_over_the_box_capacity_is_flagged_and_written_empty():
    from pdanet_amd import frame_stage as fs, _lib
    lib = _lib.load()
    rng = np.random.default_rng(22)
    n, dev = 5000, "cuda"
    pts = torch.from_numpy(_random_scans(rng, 2, n).reshape(-1, 4)).to(dev)
    offs = torch.tensor([0, n, 2 * n], dtype=torch.int64, device=dev)
    m0, m1 = 3, fs.MAX_BOXES_PER_FRAME + 1
    bx = np.concatenate([rng.uniform(-20, 20, (m0 + m1, 2)), np.zeros((m0 + m1, 1)), np.full((m0 + m1, 3), 30.0), np.zeros((m0 + m1, 1))], 1)
    boxes = torch.from_numpy(bx.astype(np.float32)).to(dev)
    centre = torch.from_numpy(np.ascontiguousarray(bx[:, :3])).to(dev)
    boffs = torch.tensor([0, m0, m0 + m1], dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="more than 256 boxes"):
        fs.gt_extract((pts, offs, n), boxes, boffs, centre)
    obj_points, obj_offs, counts, info = fs.gt_extract((pts, offs, n), boxes, boffs, centre, check=False)
    info = info.cpu().numpy()
    assert info[0].tolist() == [n, m0, 0, 0] and info[1, 3] == fs.STATUS_OVER_BOXES and info[1, 1] == m1
    c = counts.cpu().numpy()
    assert (c[:m0] > 0).all() and (c[m0:] == 0).all() and obj_points.shape[0] == c[:m0].sum()
    # the raw entries with guarded buffers: nothing beyond counts, the workspace rows or the output rows is written
    m, total, guard = m0 + m1, int(c.sum()), 64
    ws_bytes = lib.pda_gt_extract_workspace_bytes(2, i64(n), i64(m))
    ws = torch.full((ws_bytes + 256,), 0x5A, dtype=torch.uint8, device=dev)
    cnt = torch.full((m + guard,), -7, dtype=torch.int32, device=dev)
    inf = torch.full((2 * 4 + guard,), -7, dtype=torch.int32, device=dev)
    out = torch.full((total + guard, 4), -7.0, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    head = (pts.data_ptr(), offs.data_ptr(), i64(2 * n), 2, 4, i64(n), boxes.data_ptr(), boffs.data_ptr(), i64(m))
    assert lib.pda_gt_extract_count(*head, cnt.data_ptr(), inf.data_ptr(), ws.data_ptr(), st) == 0
    assert lib.pda_gt_extract_write(*head, centre.data_ptr(), obj_offs.data_ptr(), out.data_ptr(), i64(total), inf.data_ptr(),
                                    ws.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert (cnt[m:] == -7).all() and (inf[8:] == -7).all() and (out[total:] == -7.0).all() and (ws[ws_bytes:] == 0x5A).all()
    assert torch.equal(cnt[:m], counts) and torch.equal(out[:total], obj_points) and inf[7].item() == fs.STATUS_OVER_BOXES
    # an output smaller than what was counted drops rows and says so
    small = torch.full((total, 4), -7.0, dtype=torch.float32, device=dev)
    assert lib.pda_gt_extract_write(*head, centre.data_ptr(), obj_offs.data_ptr(), small.data_ptr(), i64(total - 10), inf.data_ptr(),
                                    ws.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert (small[total - 10:] == -7.0).all() and inf[3].item() & fs.STATUS_OVER_CAP
