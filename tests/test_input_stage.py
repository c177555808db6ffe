"""The input stage on the device (pdanet_amd.data_processor, csrc/input_stage.hip): ragged raw scenes -> the collated
batch, against the reference's DataProcessor + collate_batch recorded in tests/golden/input_stage.npz
(tests/golden/make_input_golden.py), plus the seeded mode's invariants and statistics, the no-host-read path, graph
capture and the detector fed from it."""
import ctypes
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "input_stage.npz")
TAGS = ("once", "kitti")
i64 = ctypes.c_int64


def _golden():
    return dict(np.load(GOLDEN))


def _rows(g, tag, key):
    off = g["%s_%s_offsets" % (tag, key)]
    v = g["%s_%s" % (tag, key)]
    return [v[off[b]:off[b + 1]] for b in range(len(off) - 1)]


def _cfg(k, shuffle_train=True, shuffle_test=False):
    return [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
            {"NAME": "sample_points", "NUM_POINTS": {"train": k, "test": k}},
            {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": shuffle_train, "test": shuffle_test}}]


# ---- a numpy statement of the stage in this test's own words --------------------------------------------------------------
def _expected(raw, offs, rng6, k, picks, perm1s, perm2s, raw_boxes, box_offs, training):
    lo, hi = rng6[:3].astype(np.float32), rng6[3:].astype(np.float32)
    rows, kept = [], []
    for b in range(len(offs) - 1):
        p = raw[offs[b]:offs[b + 1]]
        keep = (p[:, 0] >= lo[0]) & (p[:, 0] <= hi[0]) & (p[:, 1] >= lo[1]) & (p[:, 1] <= hi[1])
        q = p[keep]
        n = len(q)
        depth = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])     # float32 throughout
        close = depth < np.float32(40.0)
        close_at, far_at = np.flatnonzero(close), np.flatnonzero(~close)
        if n <= k:
            order = np.concatenate([np.arange(n), picks[b][:k - n]])
        elif len(far_at) < k:
            order = np.concatenate([close_at[picks[b][:k - len(far_at)]], far_at])
        else:
            order = picks[b][:k]
        order = order[perm1s[b]]
        if perm2s[b] is not None and len(perm2s[b]):
            order = order[perm2s[b]]
        rows.append(np.concatenate([np.full((k, 1), b, np.float32), q[order]], axis=1))
        bx = raw_boxes[box_offs[b]:box_offs[b + 1]]
        if training:
            half = bx[:, 3:6] * np.float32(0.5)
            sx = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float32)
            sy = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float32)
            sz = np.array([-1, -1, -1, -1, 1, 1, 1, 1], np.float32)
            lx, ly, lz = half[:, :1] * sx, half[:, 1:2] * sy, half[:, 2:3] * sz
            cos, sin = np.cos(bx[:, 6:7]), np.sin(bx[:, 6:7])
            x = (lx * cos - ly * sin) + bx[:, 0:1]
            y = (lx * sin + ly * cos) + bx[:, 1:2]
            z = lz + bx[:, 2:3]
            ins = (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1]) & (z >= lo[2]) & (z <= hi[2])
            bx = bx[ins.sum(1) >= 1]
        kept.append(bx)
    cap = max(len(x) for x in kept)
    gt = np.zeros((len(kept), cap, raw_boxes.shape[1]), np.float32)
    for b, x in enumerate(kept):
        gt[b, :len(x)] = x
    return np.concatenate(rows), gt, np.array([len(x) for x in kept], np.int32)


@pytest.mark.parametrize("tag", TAGS)
def test_numpy_statement_reproduces_the_reference_from_its_draws(tag):
    g = _golden()
    perm2 = _rows(g, tag, "perm2") if bool(g[tag + "_training"]) else [None] * (len(g[tag + "_offsets"]) - 1)
    pts, gt, kept = _expected(g[tag + "_points_raw"], g[tag + "_offsets"], g[tag + "_range"], int(g["num_points"]),
                              _rows(g, tag, "pick"), _rows(g, tag, "perm1"), perm2, g[tag + "_boxes_raw"],
                              g[tag + "_box_offsets"], bool(g[tag + "_training"]))
    assert np.array_equal(pts, g[tag + "_ref_points"])
    assert np.array_equal(gt, g[tag + "_ref_gt_boxes"])
    assert np.array_equal(kept, g[tag + "_ref_kept"])


def test_fixture_covers_the_cases():
    g = _golden()
    k = int(g["num_points"])
    seen = set()
    for tag in TAGS:
        raw, offs, rng6 = g[tag + "_points_raw"], g[tag + "_offsets"], g[tag + "_range"]
        for b in range(len(offs) - 1):
            p = raw[offs[b]:offs[b + 1]]
            m = (p[:, 0] >= rng6[0]) & (p[:, 0] <= rng6[3]) & (p[:, 1] >= rng6[1]) & (p[:, 1] <= rng6[4])
            q = p[m]
            n_far = int((np.linalg.norm(q[:, :3], axis=1) >= 40.0).sum())
            n = len(q)
            seen.add("A" if n > k and n_far < k else "B" if n > k else "C" if n < k else "n==k")
            if n > k and n_far == 0:
                seen.add("A, no far point")
            if m.mean() < 0.5:
                seen.add("mostly outside")
            if np.any(p[:, 0] == rng6[0]) and np.any(p[:, 1] == rng6[4]):
                seen.add("on the limits")
            d = np.linalg.norm(p[:, :3].astype(np.float64), axis=1)
            if np.sum(np.abs(d - 40.0) < 2e-5) >= 50:
                seen.add("40 m sphere")
        seen.add("C=%d" % raw.shape[1])
        seen.add("training" if bool(g[tag + "_training"]) else "test")
    assert seen >= {"A", "B", "C", "n==k", "A, no far point", "mostly outside", "on the limits", "40 m sphere", "C=4", "C=5",
                    "training", "test"}
    kept = g["once_ref_kept"]
    assert kept[-1] == 0 and 0 < kept[0] < np.diff(g["once_box_offsets"])[0]      # all outside / partly removed


# ---- C ABI without a GPU ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pdanet_amd import build, _lib
    build.build()
    return _lib.load()


def test_argument_validation_without_gpu(lib):
    rng = (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    u64 = ctypes.c_uint64
    assert lib.pda_input_stage_workspace_bytes(2, i64(1000)) >= 2 * 2 * 1000 * 4
    assert lib.pda_input_stage_workspace_bytes(0, i64(1000)) >= 0
    assert lib.pda_input_stage_workspace_bytes(-1, i64(1000)) == -1
    assert lib.pda_input_stage_workspace_bytes(2, i64(0)) == -1
    assert lib.pda_input_stage_workspace_bytes(2, i64(1 << 31)) == -1
    stage = lambda *a: lib.pda_input_stage(*a)       # noqa: E731
    # sizes are checked before any pointer is used
    assert stage(None, None, i64(0), 0, 4, i64(10), rng, 16, None, None, None, u64(0), 0, None, None, None, None) == 0   # no scene
    assert stage(None, None, i64(0), 2, 2, i64(10), rng, 16, None, None, None, u64(0), 0, None, None, None, None) == 1
    assert b"bad size" in lib.pda_last_error()
    assert stage(None, None, i64(0), 2, 4, i64(10), rng, 0, None, None, None, u64(0), 0, None, None, None, None) == 1
    assert stage(None, None, i64(0), 2, 4, i64(0), rng, 16, None, None, None, u64(0), 0, None, None, None, None) == 1
    assert stage(None, None, i64(-1), 2, 4, i64(10), rng, 16, None, None, None, u64(0), 0, None, None, None, None) == 1
    assert stage(None, None, i64(0), 2, 4, i64(10), rng, 16, None, None, None, u64(0), 2, None, None, None, None) == 1
    assert stage(None, None, i64(10), 2, 4, i64(10), rng, 16, None, None, None, u64(0), 0, None, None, None, None) == 1
    assert b"null" in lib.pda_last_error()
    # the mode checks: every required pointer stays NULL, so none of these calls can reach a launch whatever the order of
    # the checks; the draw pointers only need to be non-NULL (a host buffer, never read)
    host = ctypes.cast((ctypes.c_int32 * 4)(), ctypes.c_void_p)
    args = lambda pick, p1, p2, sh: (None, None, i64(10), 2, 4, i64(10), rng, 16, pick, p1, p2, u64(0), sh, None, None, None, None)  # noqa: E731
    assert stage(*args(host, None, None, 0)) == 1 and b"pick and perm1" in lib.pda_last_error()
    assert stage(*args(host, host, None, 1)) == 1 and b"perm2" in lib.pda_last_error()
    assert stage(*args(host, host, host, 0)) == 1 and b"perm2" in lib.pda_last_error()
    assert stage(*args(None, None, host, 1)) == 1 and b"seeded" in lib.pda_last_error()
    assert stage(*args(host, host, host, 1)) == 1 and b"null" in lib.pda_last_error()        # a consistent mode, no buffers
    boxes = lambda *a: lib.pda_input_boxes(*a)      # noqa: E731
    assert boxes(None, None, i64(0), 0, 8, 4, rng, 1, None, None, None) == 0
    assert boxes(None, None, i64(0), 2, 6, 4, rng, 1, None, None, None) == 1 and b"bad size" in lib.pda_last_error()
    assert boxes(None, None, i64(0), 2, 8, -1, rng, 1, None, None, None) == 1
    assert boxes(None, None, i64(0), 2, 8, 4, rng, 9, None, None, None) == 1
    assert boxes(None, None, i64(3), 2, 8, 4, rng, 1, None, None, None) == 1 and b"null" in lib.pda_last_error()
    assert boxes(None, None, i64(0), 2, 8, 0, rng, 1, None, None, None) == 1 and b"null" in lib.pda_last_error()


# ---- configuration ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yaml_name,k", [("once_pda_ssd.yaml", 60000), ("kitti_pda_ssd.yaml", 16384)])
def test_data_processor_reads_the_repo_yamls(yaml_name, k):
    from pdanet_amd import config, data_processor
    cfg = config.load_yaml(yaml_name)
    for training in (True, False):
        dp = data_processor.from_config(cfg, training)
        assert dp.num_points == k and dp.mask_points and dp.min_num_corners == 1
        assert dp.shuffle == training and dp.remove_outside_boxes == training
        assert np.array_equal(dp.point_cloud_range, np.array(cfg.DATA_CONFIG.POINT_CLOUD_RANGE, np.float32))


def test_data_processor_refuses_what_it_cannot_run():
    from pdanet_amd.data_processor import DataProcessor
    rng6 = [0, -40, -3, 70.4, 40, 1]
    cfg = _cfg(16384)
    cfg[1]["NUM_POINTS"] = {"train": -1, "test": -1}
    with pytest.raises(ValueError, match="NUM_POINTS"):
        DataProcessor(cfg, rng6, True, 4)
    with pytest.raises(NotImplementedError):
        DataProcessor(_cfg(100) + [{"NAME": "transform_points_to_voxels", "VOXEL_SIZE": [0.1, 0.1, 0.1]}], rng6, True, 4)
    with pytest.raises(NotImplementedError):
        DataProcessor([_cfg(100)[2], _cfg(100)[1]], rng6, True, 4)
    with pytest.raises(ValueError):
        DataProcessor(_cfg(100)[:1], rng6, True, 4)


# ---- on the GPU --------------------------------------------------------------------------------------------------------------
def _dp(k, rng6, training, c=4, shuffle=True):
    from pdanet_amd.data_processor import DataProcessor
    return DataProcessor(_cfg(k, shuffle_train=shuffle), rng6, training, c)


def _split(raw, offs):
    return [raw[offs[b]:offs[b + 1]] for b in range(len(offs) - 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_explicit_draws_give_the_reference_batch(tag):
    g = _golden()
    training = bool(g[tag + "_training"])
    dp = _dp(int(g["num_points"]), g[tag + "_range"], training, c=g[tag + "_points_raw"].shape[1])
    draws = {"pick": _rows(g, tag, "pick"), "perm1": _rows(g, tag, "perm1")}
    if training:
        draws["perm2"] = _rows(g, tag, "perm2")
    scenes = _split(g[tag + "_points_raw"], g[tag + "_offsets"])
    boxes = _split(g[tag + "_boxes_raw"], g[tag + "_box_offsets"])
    bd = dp(scenes, boxes, draws=draws)
    assert bd["batch_size"] == len(scenes)
    got = bd["points"].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), g[tag + "_ref_points"].view(np.uint32))
    assert np.array_equal(bd["gt_boxes"].cpu().numpy(), g[tag + "_ref_gt_boxes"])
    info = bd["input_info"].cpu().numpy()
    assert np.array_equal(info[:, 2], g[tag + "_ref_kept"])
    assert (info[:, 3] == 0).all()
    # the same draws with device inputs and a fixed capacity: the same batch, zero-padded further
    pts = torch.from_numpy(g[tag + "_points_raw"]).cuda()
    offs = torch.from_numpy(g[tag + "_offsets"]).cuda()
    bx = torch.from_numpy(g[tag + "_boxes_raw"]).cuda()
    boffs = torch.from_numpy(g[tag + "_box_offsets"]).cuda()
    bd2 = dp((pts, offs, int(np.diff(g[tag + "_offsets"]).max())), (bx, boffs), max_gt=16, draws=draws)
    assert torch.equal(bd2["points"], bd["points"])
    ref = g[tag + "_ref_gt_boxes"]
    gt2 = bd2["gt_boxes"].cpu().numpy()
    assert gt2.shape == (len(scenes), 16, ref.shape[2])
    assert np.array_equal(gt2[:, :ref.shape[1]], ref) and not gt2[:, ref.shape[1]:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_collate_batch_of_reference_shaped_dicts(tag):
    """data_processor.collate_batch on the reference's per-scene dicts (numpy points / gt_boxes, a frame_id string): the
    fixture's collated points and boxes, and the same boxes padded further with max_gt; CPU tensors in give the same."""
    from pdanet_amd.data_processor import collate_batch
    g = _golden()
    ref_pts, ref_gt, kept = g[tag + "_ref_points"], g[tag + "_ref_gt_boxes"], g[tag + "_ref_kept"]
    B = len(kept)
    scenes = [{"points": ref_pts[ref_pts[:, 0] == b, 1:].copy(), "gt_boxes": ref_gt[b, :kept[b]].copy(),
               "frame_id": "%s_%06d" % (tag, b)} for b in range(B)]
    out = collate_batch(scenes)
    assert out["batch_size"] == B and out["points"].is_cuda and out["gt_boxes"].is_cuda
    assert np.array_equal(out["points"].cpu().numpy(), ref_pts)
    assert np.array_equal(out["gt_boxes"].cpu().numpy(), ref_gt)
    assert out["frame_id"].tolist() == ["%s_%06d" % (tag, b) for b in range(B)]
    wide = collate_batch(scenes, max_gt=16)["gt_boxes"].cpu().numpy()
    assert wide.shape == (B, 16, ref_gt.shape[2])
    assert np.array_equal(wide[:, :ref_gt.shape[1]], ref_gt) and not wide[:, ref_gt.shape[1]:].any()
    as_tensors = [{"points": torch.from_numpy(d["points"]), "gt_boxes": torch.from_numpy(d["gt_boxes"])} for d in scenes]
    out_t = collate_batch(as_tensors)
    assert torch.equal(out_t["points"], out["points"]) and torch.equal(out_t["gt_boxes"], out["gt_boxes"])
    with pytest.raises(ValueError, match="max_gt"):
        collate_batch(scenes, max_gt=int(kept.max()) - 1)


def _scene(rng, n_near, n_far, n_out, first_id, c=4):
    """(n, c) points of a ONCE-like range, feature 0 = a unique id (exact in float32)."""
    r = np.concatenate([rng.uniform(2, 39, n_near), rng.uniform(41, 74, n_far)])
    a = rng.uniform(-np.pi, np.pi, r.size)
    p = np.zeros((n_near + n_far + n_out, c), np.float32)
    p[:r.size, 0] = r * np.cos(a)
    p[:r.size, 1] = r * np.sin(a)
    p[:r.size, 2] = rng.uniform(-2, 1, r.size)
    p[r.size:, 0] = rng.uniform(80, 100, n_out)
    p[r.size:, 1] = rng.uniform(-70, 70, n_out)
    p[:, 3] = np.arange(first_id, first_id + p.shape[0])
    return p[rng.permutation(p.shape[0])]


ONCE_RANGE = [-75.2, -75.2, -5.0, 75.2, 75.2, 3.0]


@pytest.mark.gpu
def test_seeded_mode_invariants_at_full_size():
    rng = np.random.default_rng(5)
    k = 60000
    dp = _dp(k, ONCE_RANGE, True)
    batches = {"A,C": [_scene(rng, 60000, 25000, 15000, 0), _scene(rng, 30000, 12000, 58000, 200000)],
               "B": [_scene(rng, 10000, 70000, 20000, 0), _scene(rng, 1000, 90000, 9000, 200000)]}
    for name, scenes in batches.items():
        bd = dp(scenes, seed=1234)
        out = bd["points"].cpu().numpy()
        info = bd["input_info"].cpu().numpy()
        assert out.shape == (2 * k, 5)
        for b, p in enumerate(scenes):
            rows = out[b * k:(b + 1) * k]
            assert (rows[:, 0] == b).all()
            ids = rows[:, 4].astype(np.int64)
            first = int(p[:, 3].min())
            p = p[np.argsort(p[:, 3])]                              # row r of p now holds id first + r
            src = p[ids - first]                                    # the raw row each output row names
            assert np.array_equal(src, rows[:, 1:])                 # a verbatim copy of that row
            inside = p[:, 0] <= 75.2
            far = inside & (np.linalg.norm(p[:, :3], axis=1) >= 40.0)
            n, n_far = int(inside.sum()), int(far.sum())
            assert info[b].tolist()[:2] == [n, n_far] and info[b, 3] == 0
            assert inside[ids - first].all()
            counts = np.bincount(ids - first, minlength=len(p))
            if n > k:
                assert counts.max() == 1                            # without replacement (A and B)
                if n_far < k:
                    assert (counts[far] == 1).all()                 # (A) every far point exactly once
            else:
                assert (counts[inside] >= 1).all() and counts.sum() == k     # (C) every masked point, then extras
    again = dp(batches["A,C"], seed=1234)["points"]
    assert torch.equal(again, dp(batches["A,C"], seed=1234)["points"])
    assert not torch.equal(again, dp(batches["A,C"], seed=1235)["points"])
    torch.manual_seed(3)
    a = dp(batches["A,C"])["points"]
    torch.manual_seed(3)
    assert torch.equal(a, dp(batches["A,C"])["points"])


@pytest.mark.gpu
def test_seeded_mode_statistics():
    """1000 near + 100 far points, 400 kept: case A picks 300 of the near points.  Over 400 seeds each near point's
    inclusion count is Binomial(400, 0.3) (6 sigma), and the source of output slot 0 is uniform over the 400 kept points:
    chi-square over 11 cells (far, 10 groups of 100 near points), 10 degrees of freedom, p > 1e-4 <=> statistic < 35.56."""
    rng = np.random.default_rng(9)
    p = _scene(rng, 1000, 100, 0, 0)
    dp = _dp(400, ONCE_RANGE, True)
    is_far = np.linalg.norm(p[np.argsort(p[:, 3]), :3], axis=1) >= 40.0       # by id
    near_ids = np.flatnonzero(~is_far)
    incl = np.zeros(len(p), np.int64)
    cells = np.zeros(11, np.int64)
    for s in range(400):
        ids = dp([p], seed=s)["points"][:, 4].cpu().numpy().astype(np.int64)
        assert is_far[ids].sum() == 100 and len(set(ids.tolist())) == 400
        incl[ids] += 1
        f = ids[0]
        cells[10 if is_far[f] else np.searchsorted(near_ids, f) // 100] += 1
    mean, sd = 400 * 0.3, np.sqrt(400 * 0.3 * 0.7)
    assert np.abs(incl[~is_far] - mean).max() < 6 * sd
    assert (incl[is_far] == 400).all()
    expect = np.array([400 * 0.75 / 10] * 10 + [400 * 0.25])
    chi2 = float(((cells - expect) ** 2 / expect).sum())
    assert chi2 < 35.56, (chi2, cells.tolist())


def _device_batch(rng, sizes, n_cap, boxes_per_scene):
    parts = [_scene(rng, int(s * 0.6), int(s * 0.3), s - int(s * 0.6) - int(s * 0.3), 100000 * b) for b, s in enumerate(sizes)]
    packed = torch.zeros((len(sizes) * n_cap, 4), dtype=torch.float32, device="cuda")
    flat = np.concatenate(parts)
    packed[:len(flat)] = torch.from_numpy(flat).cuda()
    offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device="cuda")
    bx = []
    for m in boxes_per_scene:
        b = np.zeros((m, 8), np.float32)
        b[:, 0:2] = rng.uniform(-60, 60, (m, 2))
        b[:, 2] = -1.0
        b[:, 3:6] = [4.0, 1.8, 1.6]
        b[:, 6] = rng.uniform(-3, 3, m)
        b[:, 7] = 1
        b[0, 0] = 90.0                                  # one box per scene outside the range
        bx.append(b)
    boxes = torch.zeros((len(sizes) * 16, 8), dtype=torch.float32, device="cuda")
    fb = np.concatenate(bx)
    boxes[:len(fb)] = torch.from_numpy(fb).cuda()
    boffs = torch.tensor(np.concatenate([[0], np.cumsum(boxes_per_scene)]), dtype=torch.int64, device="cuda")
    return packed, offs, boxes, boffs


@pytest.mark.gpu
def test_no_host_read_path_and_graph_capture():
    rng = np.random.default_rng(11)
    n_cap, k = 30000, 16384
    dp = _dp(k, ONCE_RANGE, True)
    packed, offs, boxes, boffs = _device_batch(rng, [26000, 9000], n_cap, [7, 12])
    torch.cuda.synchronize()
    dp((packed, offs, n_cap), (boxes, boffs), max_gt=16, seed=77, check=False)      # loads the kernels
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        bd = dp((packed, offs, n_cap), (boxes, boffs), max_gt=16, seed=77, check=False)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    info = bd["input_info"].cpu().numpy()
    assert info[:, 2].tolist() == [6, 11] and (info[:, 3] == 0).all()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = dp((packed, offs, n_cap), (boxes, boffs), max_gt=16, seed=77, check=False)
    g.replay()
    assert torch.equal(static["points"], bd["points"]) and torch.equal(static["gt_boxes"], bd["gt_boxes"])
    # new scenes of other sizes (within n_cap) written into the static inputs
    p2, o2, b2, bo2 = _device_batch(np.random.default_rng(12), [12000, 29999], n_cap, [3, 9])
    packed.copy_(p2); offs.copy_(o2); boxes.copy_(b2); boffs.copy_(bo2)
    g.replay()
    eager = dp((packed, offs, n_cap), (boxes, boffs), max_gt=16, seed=77, check=False)
    torch.cuda.synchronize()
    assert torch.equal(static["points"], eager["points"]) and torch.equal(static["gt_boxes"], eager["gt_boxes"])
    assert torch.equal(static["input_info"], eager["input_info"])
    assert static["input_info"][:, 2].tolist() == [2, 8]
    # a scene with no point in range is flagged on the no-read path and raises on the checked path
    o3 = torch.tensor([0, 5, 5 + 9000], dtype=torch.int64, device="cuda")
    packed[:5, 0] = 200.0
    bd3 = dp((packed, o3, n_cap), (boxes, boffs), max_gt=16, seed=1, check=False)
    assert bd3["input_info"][0, 3].item() & 1 and not bd3["points"][:k, 1:].any()
    with pytest.raises(ValueError, match="no point"):
        dp((packed, o3, n_cap), (boxes, boffs), max_gt=16, seed=1)
    with pytest.raises(ValueError, match="max_gt"):
        dp((packed, offs, n_cap), (boxes, boffs), max_gt=4, seed=1)


# ---- the detector fed from the stage -----------------------------------------------------------------------------------------
KITTI_RANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]


def _kitti_raw(rng):
    def scene(n, n_out):
        p = np.zeros((n, 4), np.float32)
        p[:, 0] = rng.uniform(2, 68, n)
        p[:, 1] = rng.uniform(-38, 38, n)
        p[:, 2] = rng.uniform(-2.5, 0.5, n)
        p[:, 3] = rng.uniform(0, 1, n)
        p[:n_out, 0] = rng.uniform(-30, -1, n_out)                 # behind the sensor: outside the range
        return p[rng.permutation(n)]

    def boxes(m):
        b = np.zeros((m, 8), np.float32)
        b[:, 0] = rng.uniform(5, 65, m)
        b[:, 1] = rng.uniform(-35, 35, m)
        b[:, 2] = -1.0
        b[:, 3:6] = [3.9, 1.6, 1.5]
        b[:, 6] = rng.uniform(-np.pi, np.pi, m)
        b[:, 7] = rng.integers(1, 4, m)
        b[0, 0] = -20.0                                           # outside
        return b

    return [scene(30000, 10000), scene(14000, 0)], [boxes(7), boxes(12)]


def _kitti_model():
    from pdanet_amd import data_processor, detector
    torch.manual_seed(7)
    model, cfg = detector.build_detector("kitti_pda_ssd.yaml")
    return model.cuda(), cfg, data_processor


@pytest.mark.gpu
def test_detector_trains_and_infers_on_stage_output():
    model, cfg, data_processor = _kitti_model()
    scenes, boxes = _kitti_raw(np.random.default_rng(21))
    dp = data_processor.from_config(cfg, training=True)
    bd = dp(scenes, boxes, max_gt=32, seed=5)
    assert bd["points"].shape == (2 * 16384, 5) and bd["gt_boxes"].shape == (2, 32, 8)
    assert bd["input_info"][:, 2].tolist() == [6, 11]
    model.train()
    ret, tb, _ = model(bd)
    assert torch.isfinite(ret["loss"])
    ret["loss"].backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    # the head loss does not depend on the box capacity: max-in-batch padding (11) against 32
    model.zero_grad(set_to_none=True)
    bd_ref = dp(scenes, boxes, max_gt=None, seed=5)
    assert bd_ref["gt_boxes"].shape == (2, 11, 8)
    assert torch.equal(bd_ref["points"], bd["points"])
    with torch.no_grad():
        l32 = model(bd)[0]["loss"].item()
        l11 = model(bd_ref)[0]["loss"].item()
    print("head loss, capacity 32: %r, max-in-batch 11: %r, bitwise equal: %s" % (l32, l11, l32 == l11))
    assert l32 == pytest.approx(l11, rel=1e-6)
    model.eval()
    dpi = data_processor.from_config(cfg, training=False)
    with torch.no_grad():
        preds, _ = model(dpi(scenes, seed=6))
    assert len(preds) == 2 and all({"pred_boxes", "pred_scores", "pred_labels"} <= set(p) for p in preds)


@pytest.mark.gpu
def test_fixed_box_capacity_keeps_one_head_graph():
    model, cfg, data_processor = _kitti_model()
    model.train()
    model.graph_head = True
    dp = data_processor.from_config(cfg, training=True)
    rng = np.random.default_rng(31)
    scenes, boxes = _kitti_raw(rng)
    kept = []
    for it, nb in enumerate(((7, 12), (3, 5))):
        bd = dp(scenes, [boxes[0][:nb[0]], boxes[1][:nb[1]]], max_gt=32, seed=40 + it)
        kept.append(bd["input_info"][:, 2].tolist())
        model.zero_grad(set_to_none=True)
        ret, _, _ = model(bd)
        ret["loss"].backward()
        assert torch.isfinite(ret["loss"])
        if it == 0:
            first = model._graphed
            assert first is not None
    assert kept[0] != kept[1]
    assert model._graphed is first
