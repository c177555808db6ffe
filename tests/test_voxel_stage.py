"""Voxel down-sampling on the device (pdanet_amd.voxel_utils, pdanet_amd.data_processor's sample_points_by_voxels chain,
csrc/voxel_stage.hip) against the reference's DataProcessor + collate_batch recorded in tests/golden/voxel_sample.npz
(tests/golden/make_voxel_sample_golden.py; the voxelizer there is a plain-Python restatement of spconv's CPU loop, spconv
itself was not run), plus determinism, the seeded shuffle's statistics, the no-host-read path and the detector fed from it."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "voxel_sample.npz")
CASES = [("raw", "train"), ("raw", "test"), ("mean", "train"), ("mean", "test")]
SAMPLE_TYPE = {"raw": "raw", "mean": "mean_vfe"}
WAYMO_RANGE = [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0]
i64 = ctypes.c_int64
u64 = ctypes.c_uint64


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


def _rows(g, prefix, key):
    off = g["%s_%s_offsets" % (prefix, key)]
    v = g["%s_%s" % (prefix, key)]
    return [v[off[b]:off[b + 1]] for b in range(len(off) - 1)]


def _split(raw, offs):
    return [raw[offs[b]:offs[b + 1]] for b in range(len(offs) - 1)]


def _cfg(sample_type="raw", k=65536, voxel_size=(0.1, 0.1, 0.15), max_points=5, max_voxels=(80000, 90000), shuffle=(True, False),
         mask=True, with_shuffle=True):
    steps = []
    if mask:
        steps.append({"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True})
    if with_shuffle:
        steps.append({"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": shuffle[0], "test": shuffle[1]}})
    steps.append({"NAME": "sample_points_by_voxels", "SAMPLE_TYPE": sample_type, "VOXEL_SIZE": list(voxel_size),
                  "MAX_POINTS_PER_VOXEL": max_points, "MAX_NUMBER_OF_VOXELS": {"train": max_voxels[0], "test": max_voxels[1]},
                  "NUM_POINTS": {"train": k, "test": k}})
    return steps


def _golden_dp(g, tag, mode):
    from pdanet_amd.data_processor import DataProcessor
    cfg = _cfg(SAMPLE_TYPE[tag], int(g["num_points"]), g["voxel_size"].tolist(), int(g["max_points"]),
               tuple(int(x) for x in g["max_voxels"]))
    return DataProcessor(cfg, g["range"], mode == "train", g[tag + "_points_raw"].shape[1])


# ---- a vectorised numpy statement of the voxelizer in this test's own words -------------------------------------------------
def _assign(p, rng6, voxel_size):
    """-> the rows of p that fall into the grid, their cells (x, y, z) and their voxel numbers before the cap."""
    lo, vs = rng6[:3].astype(np.float32), np.asarray(voxel_size, np.float32)
    grid = np.round((rng6[3:6] - rng6[0:3]) / np.array(voxel_size)).astype(np.int64)
    with np.errstate(invalid="ignore"):
        f = np.floor((p[:, :3] - lo) / vs)                                   # float32 throughout
        ok = ((f >= 0) & (f < grid.astype(np.float32))).all(axis=1)          # a NaN compares false
    at = np.flatnonzero(ok)
    c = f[at].astype(np.int64)
    key = (c[:, 2] * grid[1] + c[:, 1]) * grid[0] + c[:, 0]
    uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
    number = np.empty(len(uniq), np.int64)
    number[np.argsort(first)] = np.arange(len(uniq))                         # cells in order of first appearance
    return at, c, number[inv.reshape(-1)], len(uniq)


def _voxelize_np(p, rng6, voxel_size, max_points, max_voxels):
    """-> voxels (V, max_points, C), coords (V, 3) (z, y, x), num (V), [n_in_grid, n_voxels_before_cap]."""
    at, c, v, n_before = _assign(p, rng6, voxel_size)
    by_voxel = np.argsort(v, kind="stable")
    rank = np.empty(len(v), np.int64)
    rank[by_voxel] = np.arange(len(v)) - np.searchsorted(v[by_voxel], v[by_voxel], side="left")
    n_vox = min(n_before, max_voxels)
    put = (v < max_voxels) & (rank < max_points)
    voxels = np.zeros((n_vox, max_points, p.shape[1]), np.float32)
    voxels[v[put], rank[put]] = p[at[put]]
    coords = np.zeros((n_vox, 3), np.int32)
    head = (rank == 0) & (v < max_voxels)
    coords[v[head]] = c[head][:, ::-1]
    num = np.minimum(np.bincount(v[v < max_voxels], minlength=n_vox), max_points).astype(np.int32)
    return voxels, coords, num, [len(at), n_before]


def _expected_points(g, tag, mode):
    """The whole chain from the recorded draws -> the collated points and [n_masked, n_in_grid, n_voxels_before_cap]."""
    rng6, k, training = g["range"], int(g["num_points"]), mode == "train"
    prefix = "%s_%s" % (tag, mode)
    picks, perm1s, perm0s = _rows(g, prefix, "pick"), _rows(g, prefix, "perm1"), _rows(g, prefix, "perm0")
    max_voxels = int(g["max_voxels"][0 if training else 1])
    out, counts = [], []
    for b, p in enumerate(_split(g[tag + "_points_raw"], g[tag + "_offsets"])):
        q = p[(p[:, 0] >= rng6[0]) & (p[:, 0] <= rng6[3]) & (p[:, 1] >= rng6[1]) & (p[:, 1] <= rng6[4])]
        n_masked = len(q)
        if training:
            q = q[perm0s[b]]
        voxels, _, num, cnt = _voxelize_np(q, rng6, g["voxel_size"], int(g["max_points"]), max_voxels)
        counts.append([n_masked] + cnt)
        if tag == "mean":
            rows = voxels.sum(axis=1) / num[:, None]                          # float32 sums, float64 quotient
        else:
            rows = voxels[:, 0]
        depth = np.sqrt((rows[:, 0] * rows[:, 0] + rows[:, 1] * rows[:, 1]) + rows[:, 2] * rows[:, 2])   # in the rows' type
        n = len(rows)
        close_at, far_at = np.flatnonzero(depth < 40.0), np.flatnonzero(~(depth < 40.0))
        if n <= k:
            order = np.concatenate([np.arange(n), picks[b][:k - n]])
        elif len(far_at) < k:
            order = np.concatenate([close_at[picks[b][:k - len(far_at)]], far_at])
        else:
            order = picks[b][:k]
        order = order[perm1s[b]]
        out.append(np.concatenate([np.full((k, 1), b, np.float64), rows[order]], axis=1).astype(np.float32))
    return np.concatenate(out), np.array(counts, np.int32)


@pytest.mark.parametrize("tag,mode", CASES)
def test_numpy_statement_reproduces_the_reference_from_its_draws(tag, mode):
    g = _golden()
    pts, counts = _expected_points(g, tag, mode)
    ref = g["%s_%s_ref_points" % (tag, mode)]
    assert np.array_equal(pts.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(counts, g["%s_%s_ref_counts" % (tag, mode)])


def test_fixture_covers_the_cases():
    g = _golden()
    rng6, k, mp = g["range"], int(g["num_points"]), int(g["max_points"])
    lo, vs = rng6[:3].astype(np.float64), g["voxel_size"]
    seen = set()
    for tag, mode in CASES:
        max_voxels = int(g["max_voxels"][0 if mode == "train" else 1])
        perm0s = _rows(g, "%s_%s" % (tag, mode), "perm0")
        for b, p in enumerate(_split(g[tag + "_points_raw"], g[tag + "_offsets"])):
            assert 3000 <= len(p) <= 6000 and p.shape[1] == 5
            q = p[(p[:, 0] >= rng6[0]) & (p[:, 0] <= rng6[3]) & (p[:, 1] >= rng6[1]) & (p[:, 1] <= rng6[4])]
            if mode == "train":
                assert np.array_equal(np.sort(perm0s[b]), np.arange(len(q)))
                q = q[perm0s[b]]
            voxels, _, num, (n_in, n_before) = _voxelize_np(q, rng6, vs, 64, max_voxels)       # 64: the full counts
            rows = voxels[:, :mp].sum(axis=1) / np.minimum(num, mp)[:, None] if tag == "mean" else voxels[:, 0]
            d = np.linalg.norm(rows[:, :3].astype(np.float64), axis=1)
            n, n_far = len(rows), int((d >= 40.0).sum())
            seen.add((tag, "A" if n > k and n_far < k else "B" if n > k else "C"))
            if (num == 1).any() and (num == mp).any() and (num > mp).any():
                seen.add((tag, "1, exactly 5 and more than 5 points"))
            if n_before > max_voxels:
                # after the cap is reached, later points fall into existing voxels and into refused ones
                _, _, v, _ = _assign(q, rng6, vs)
                full_at = int(np.flatnonzero(v == max_voxels - 1)[0])
                later = v[full_at + 1:]
                assert (later < max_voxels).any() and (later >= max_voxels).any()
                assert (later[np.flatnonzero(later >= max_voxels)[0]:] < max_voxels).any()
                seen.add((tag, "cap hit"))
            if tag == "mean":
                assert np.abs(d - 40.0).min() > 1e-4
            elif np.sum(np.abs(d - 40.0) < 2e-5) >= 50 and n > k and n_far < k:
                seen.add((tag, "40 m sphere in case A"))
            if np.any(p[:, 0] == rng6[3]) and np.any(p[:, 1] == rng6[4]) and np.any(p[:, 2] > rng6[5]) and np.any(p[:, 2] < rng6[2]):
                seen.add((tag, "x == xmax, y == ymax, z outside"))
            for axis in range(3):
                face = np.float32(lo[axis] + np.arange(1, 256) * vs[axis])
                on = np.isin(p[:, axis], face).sum()
                below = np.isin(p[:, axis], np.nextafter(face, np.float32(-1e9))).sum()
                above = np.isin(p[:, axis], np.nextafter(face, np.float32(1e9))).sum()
                if on >= 3 and below >= 3 and above >= 3:
                    seen.add((tag, "faces of axis %d" % axis))
    for tag in ("raw", "mean"):
        assert {c for t, c in seen if t == tag} >= {"A", "B", "C", "1, exactly 5 and more than 5 points", "cap hit",
                                                     "x == xmax, y == ymax, z outside", "faces of axis 0", "faces of axis 1",
                                                     "faces of axis 2"}
    assert ("raw", "40 m sphere in case A") in seen
    assert os.path.getsize(GOLDEN) <= max(os.path.getsize(os.path.join(HERE, "golden", f)) for f in os.listdir(os.path.join(HERE, "golden")))


# ---- configuration -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
def test_data_processor_reads_the_waymo_shaped_list(training):
    from pdanet_amd.data_processor import DataProcessor
    dp = DataProcessor(_cfg(), WAYMO_RANGE, training, 5)
    assert dp.num_points == 65536 and dp.sample_type == "raw" and dp.mask_points
    assert dp.shuffle_first == training and dp.shuffle is False and dp.remove_outside_boxes == training
    assert dp.voxel.max_points == 5 and dp.voxel.max_voxels == (80000 if training else 90000)
    assert dp.voxel.grid.tolist() == [1504, 1504, 40]
    assert np.array_equal(dp.voxel.voxel_size, np.array([0.1, 0.1, 0.15], np.float32))
    mean = DataProcessor(_cfg("mean_vfe", mask=False, with_shuffle=False), WAYMO_RANGE, training, 5)
    assert mean.sample_type == "mean_vfe" and not mean.mask_points and not mean.shuffle_first
    no_type = _cfg()
    del no_type[2]["SAMPLE_TYPE"]
    assert DataProcessor(no_type, WAYMO_RANGE, training, 5).sample_type == "raw"


def test_data_processor_refuses_what_it_cannot_run():
    from pdanet_amd.data_processor import DataProcessor
    with pytest.raises(ValueError, match="NUM_POINTS"):
        DataProcessor(_cfg(k=-1), WAYMO_RANGE, True, 5)
    vox = _cfg()
    sample = {"NAME": "sample_points", "NUM_POINTS": {"train": 100, "test": 100}}
    with pytest.raises(NotImplementedError):                          # the voxel step in front of the shuffle
        DataProcessor([vox[0], vox[2], vox[1]], WAYMO_RANGE, True, 5)
    with pytest.raises(NotImplementedError):                          # both sampling steps
        DataProcessor(vox + [sample], WAYMO_RANGE, True, 5)
    with pytest.raises(NotImplementedError):
        DataProcessor([vox[0], sample, vox[2]], WAYMO_RANGE, True, 5)
    with pytest.raises(NotImplementedError):
        DataProcessor(vox + [{"NAME": "transform_points_to_voxels", "VOXEL_SIZE": [0.1, 0.1, 0.15]}], WAYMO_RANGE, True, 5)
    with pytest.raises(NotImplementedError):                          # as before: a shuffle in front of plain sample_points
        DataProcessor([vox[1], sample], WAYMO_RANGE, True, 5)
    with pytest.raises(NotImplementedError):
        DataProcessor([vox[0], {"NAME": "calculate_grid_size", "VOXEL_SIZE": [0.1, 0.1, 0.15]}], WAYMO_RANGE, True, 5)
    with pytest.raises(ValueError):                                   # no sampling step
        DataProcessor(vox[:2], WAYMO_RANGE, True, 5)
    with pytest.raises(ValueError, match="SAMPLE_TYPE"):
        DataProcessor(_cfg("median"), WAYMO_RANGE, True, 5)


# ---- C ABI without a GPU -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pdanet_amd import build, _lib
    build.build()
    return _lib.load()


def test_argument_validation_without_gpu(lib):
    f3, f6, i3 = ctypes.c_float * 3, ctypes.c_float * 6, ctypes.c_int32 * 3
    rng, vs, grid = f6(*WAYMO_RANGE), f3(0.1, 0.1, 0.15), i3(1504, 1504, 40)
    ws = lib.pda_voxel_workspace_bytes
    assert ws(2, i64(1000), 3000, 5) >= 2 * 2048 * 8 and ws(0, i64(1000), 3000, 5) >= 0
    for bad in ((-1, i64(1000), 3000, 5), (2, i64(0), 3000, 5), (2, i64(1 << 31), 3000, 5), (2, i64(1000), 0, 5),
                (2, i64(1000), 3000, 0), (2, i64(1000), 3000, 65)):
        assert ws(*bad) == -1

    def sample(batch=2, c=5, n_total=0, n_cap=10, rng=rng, vs=vs, grid=grid, mask=1, max_voxels=8, max_points=5, mean=0, shuffle=0,
               perm0=None, poffs=None, out_cap=100):
        return lib.pda_voxel_sample(None, None, i64(n_total), batch, c, i64(n_cap), rng, vs, grid, mask, max_voxels, max_points, mean,
                                    shuffle, perm0, poffs, i64(0), u64(0), None, i64(out_cap), None, None, None, None)

    def voxelize(batch=2, c=5, n_total=0, n_cap=10, rng=rng, vs=vs, grid=grid, max_voxels=8, max_points=5):
        return lib.pda_voxelize(None, None, i64(n_total), batch, c, i64(n_cap), rng, vs, grid, max_voxels, max_points, None, None,
                                None, None, None, None)

    for entry, name in ((sample, b"pda_voxel_sample"), (voxelize, b"pda_voxelize")):
        assert entry(batch=0) == 0                                                     # no scene
        for kw in (dict(c=2), dict(n_total=-1), dict(n_cap=0), dict(max_voxels=0), dict(max_points=0), dict(max_points=65), dict(batch=-1)):
            assert entry(**kw) == 1 and b"bad size" in lib.pda_last_error() and name in lib.pda_last_error()
        assert entry(rng=None) == 1 and b"null" in lib.pda_last_error()
        assert entry(grid=None) == 1 and b"null" in lib.pda_last_error()
        # every required buffer is NULL, so a call that passes the size checks stops at the pointer check: nothing is launched
        assert entry() == 1 and b"null" in lib.pda_last_error()
        # the Waymo grid (90 240 000 cells) and the ONCE range at 0.05 m (1.45e9 cells) fit the key ...
        assert entry(vs=f3(0.05, 0.05, 0.05), grid=i3(3008, 3008, 160)) == 1 and b"null" in lib.pda_last_error()
        # ... 2^32 cells do not, nor does an axis beyond 2^24 cells, nor an empty one, nor a voxel size that is not positive
        assert entry(grid=i3(65536, 65536, 1)) == 1 and b"4294967295" in lib.pda_last_error()
        assert entry(batch=0, grid=i3(4096, 4096, 4096)) == 1 and b"4294967295" in lib.pda_last_error()
        assert entry(grid=i3((1 << 24) + 1, 2, 2)) == 1 and b"bad grid" in lib.pda_last_error()
        assert entry(grid=i3(1504, 0, 40)) == 1 and b"bad grid" in lib.pda_last_error()
        assert entry(vs=f3(0.1, 0.0, 0.15)) == 1 and b"bad grid" in lib.pda_last_error()
        assert entry(vs=f3(0.1, float("nan"), 0.15)) == 1 and b"bad grid" in lib.pda_last_error()
    for kw in (dict(mask=2), dict(mean=2), dict(shuffle=2), dict(out_cap=-1)):
        assert sample(**kw) == 1 and b"bad size" in lib.pda_last_error()
    host = ctypes.cast((ctypes.c_int64 * 4)(), ctypes.c_void_p)                       # non-NULL, never read
    assert sample(shuffle=1, perm0=host) == 1 and b"perm0" in lib.pda_last_error()
    assert sample(shuffle=1, poffs=host) == 1 and b"perm0" in lib.pda_last_error()
    assert sample(shuffle=0, perm0=host, poffs=host) == 1 and b"perm0" in lib.pda_last_error()
    assert sample(out_cap=15) == 1 and b"out_cap" in lib.pda_last_error()             # 2 scenes x min(10, 8) rows
    assert sample(shuffle=1, perm0=host, poffs=host, out_cap=16) == 1 and b"null" in lib.pda_last_error()


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------
def _draws(g, tag, mode):
    prefix = "%s_%s" % (tag, mode)
    d = {"pick": _rows(g, prefix, "pick"), "perm1": _rows(g, prefix, "perm1")}
    if mode == "train":
        d["perm0"] = _rows(g, prefix, "perm0")
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("tag,mode", CASES)
def test_explicit_draws_give_the_reference_batch(tag, mode):
    g = _golden()
    dp = _golden_dp(g, tag, mode)
    prefix = "%s_%s_" % (tag, mode)
    scenes = _split(g[tag + "_points_raw"], g[tag + "_offsets"])
    boxes = _split(g[tag + "_boxes_raw"], g[tag + "_box_offsets"])
    bd = dp(scenes, boxes, draws=_draws(g, tag, mode))
    assert bd["batch_size"] == len(scenes)
    got, ref = bd["points"].cpu().numpy(), g[prefix + "ref_points"]
    print("%s %s: %d of %d rows differ" % (tag, mode, int((got.view(np.uint32) != ref.view(np.uint32)).any(axis=1).sum()), len(ref)))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(bd["gt_boxes"].cpu().numpy(), g[prefix + "ref_gt_boxes"])
    info, vinfo = bd["input_info"].cpu().numpy(), bd["voxel_info"].cpu().numpy()
    assert np.array_equal(info[:, 2], g[prefix + "ref_kept"]) and (info[:, 3] == 0).all()
    counts = g[prefix + "ref_counts"]
    max_voxels = int(g["max_voxels"][0 if mode == "train" else 1])
    assert np.array_equal(vinfo[:, :3], counts)
    assert np.array_equal(vinfo[:, 3], np.where(counts[:, 2] > max_voxels, 16, 0))
    assert np.array_equal(info[:, 0], np.minimum(counts[:, 2], max_voxels))             # the input stage counts voxel rows
    # device inputs with a larger n_cap and a fixed box capacity: the same points
    pts, offs = torch.from_numpy(g[tag + "_points_raw"]).cuda(), torch.from_numpy(g[tag + "_offsets"]).cuda()
    bx, boffs = torch.from_numpy(g[tag + "_boxes_raw"]).cuda(), torch.from_numpy(g[tag + "_box_offsets"]).cuda()
    bd2 = dp((pts, offs, 7000), (bx, boffs), max_gt=16, draws=_draws(g, tag, mode))
    assert torch.equal(bd2["points"], bd["points"]) and torch.equal(bd2["voxel_info"], bd["voxel_info"])


def _special_scenes(g):
    """The fixture's raw scenes, an empty scene, a scene with every point outside the grid, and NaN / infinite coordinates."""
    scenes = _split(g["raw_points_raw"], g["raw_offsets"])
    outside = scenes[2][:500].copy()
    outside[:, 2] += 100.0
    odd = scenes[0][:300].copy()
    odd[5, 0], odd[9, 1], odd[17, 2], odd[40, 0], odd[41, 2] = np.nan, np.nan, np.nan, np.inf, -np.inf
    return scenes[:2] + [np.zeros((0, 5), np.float32)] + scenes[2:] + [outside, odd]


@pytest.mark.gpu
@pytest.mark.parametrize("max_voxels,max_points", [(3000, 5), (700, 1), (3500, 32)])
def test_voxel_generator_matches_the_numpy_statement(max_voxels, max_points):
    from pdanet_amd.voxel_utils import VoxelGenerator
    g = _golden()
    rng6, vs = g["range"], g["voxel_size"]
    gen = VoxelGenerator(vs.tolist(), rng6, 5, max_points, max_voxels)
    scenes = _special_scenes(g)
    want = [_voxelize_np(s, rng6, vs, max_points, max_voxels) for s in scenes]
    assert any(w[3][1] > max_voxels for w in want) and any(w[3][1] == 0 for w in want)       # capped scenes, empty ones
    packed = torch.from_numpy(np.concatenate(scenes)).cuda()
    offs = torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s in scenes])]), dtype=torch.int64, device="cuda")
    voxels, coords, num, n_vox = (t.cpu().numpy() for t in gen.generate_batch((packed, offs, max(len(s) for s in scenes))))
    assert voxels.shape == (len(scenes), max_voxels, max_points, 5) and coords.shape == (len(scenes), max_voxels, 3)
    for b, (w_vox, w_coords, w_num, _) in enumerate(want):
        v = len(w_num)
        assert n_vox[b] == v
        assert np.array_equal(voxels[b, :v].view(np.uint32), w_vox.view(np.uint32))
        assert np.array_equal(coords[b, :v], w_coords) and np.array_equal(num[b, :v], w_num)
        assert not voxels[b, v:].any() and not coords[b, v:].any() and not num[b, v:].any()
    # one scene through the reference wrapper's signature, numpy in -> numpy out, trimmed
    for b in (1, len(scenes) - 2):
        one = gen.generate(scenes[b])
        assert all(isinstance(x, np.ndarray) for x in one)
        assert np.array_equal(one[0], want[b][0]) and np.array_equal(one[1], want[b][1]) and np.array_equal(one[2], want[b][2])
    # unusable offsets are reported, not followed
    bad = torch.tensor([0, 100, 50, packed.shape[0] + 1], dtype=torch.int64, device="cuda")
    assert gen.generate_batch((packed, bad, 8000))[3].tolist() == [len(_voxelize_np(scenes[0][:100], rng6, vs, max_points, max_voxels)[2]),
                                                                   -1, -1]


def _id_scene(rng, n_cells, per_cell, first_id=0, c=5):
    """Points of n_cells distinct cells of the Waymo-like grid, per_cell[i % len] points in cell i; feature 3 = a unique id."""
    cells = rng.choice(1400 * 1400, n_cells, replace=False)
    rows, cell_of = [], []
    for i, cell in enumerate(cells):
        m = per_cell[i % len(per_cell)]
        p = np.zeros((m, c), np.float32)
        p[:, 0] = -70.0 + 0.1 * (cell % 1400) + rng.uniform(0.02, 0.08, m)
        p[:, 1] = -70.0 + 0.1 * (cell // 1400) + rng.uniform(0.02, 0.08, m)
        p[:, 2] = rng.uniform(0.12, 0.23, m)
        rows.append(p)
        cell_of += [i] * m
    p = np.concatenate(rows)
    order = rng.permutation(len(p))
    p, cell_of = p[order], np.array(cell_of)[order]
    p[:, 3] = np.arange(first_id, first_id + len(p))
    return p, cell_of


@pytest.mark.gpu
def test_two_runs_give_the_same_bits():
    from pdanet_amd.data_processor import DataProcessor
    rng = np.random.default_rng(3)
    a, _ = _id_scene(rng, 9000, (1, 2, 3, 7))
    b, _ = _id_scene(rng, 6000, (1, 6))
    for sample_type in ("raw", "mean_vfe"):
        dp = DataProcessor(_cfg(sample_type, k=8192, max_voxels=(8000, 8000), shuffle=(True, True)), WAYMO_RANGE, True, 5)
        one, two = dp([a, b], seed=99), dp([a, b], seed=99)
        assert torch.equal(one["points"], two["points"]) and torch.equal(one["voxel_info"], two["voxel_info"])
        assert one["voxel_info"][:, 2].tolist() == [9000, 6000] and one["voxel_info"][:, 3].tolist() == [16, 0]
        assert not torch.equal(one["points"], dp([a, b], seed=100)["points"])
        # explicit mode with the table as tight as it gets: n_cap = the scene size, 29250 keys' points in 65536 slots
        tight, _ = _id_scene(rng, 29250, (1,))
        assert len(tight) == 29250
        draws = {"perm0": [rng.permutation(len(tight))], "pick": [rng.choice(29250, 8192, replace=False)],
                 "perm1": [rng.permutation(8192)]}
        dpt = DataProcessor(_cfg(sample_type, k=8192, max_voxels=(40000, 40000), shuffle=(True, True), mask=False), WAYMO_RANGE, True, 5)
        pts = torch.from_numpy(tight).cuda()
        offs = torch.tensor([0, len(tight)], dtype=torch.int64, device="cuda")
        r1, r2 = dpt((pts, offs, len(tight)), draws=draws), dpt((pts, offs, len(tight)), draws=draws)
        assert torch.equal(r1["points"], r2["points"]) and r1["voxel_info"][0].tolist() == [29250, 29250, 29250, 0]
        # every cell holds one point, so the voxel rows are the shuffled points and the batch follows from the draws
        want = tight[draws["perm0"][0]][draws["pick"][0]][draws["perm1"][0]]
        assert np.array_equal(r1["points"][:, 1:].cpu().numpy(), want)


@pytest.mark.gpu
def test_seeded_shuffle_picks_each_point_of_a_voxel_uniformly():
    """250 cells with m = 2, 3, 4, 5 points in turn; NUM_POINTS = the number of cells, so every voxel row reaches the batch.  Over
    200 seeds the number of times a given point is its voxel's row is Binomial(200, 1 / m): all within 6 sigma."""
    from pdanet_amd.data_processor import DataProcessor
    rng = np.random.default_rng(8)
    per_cell = (2, 3, 4, 5)
    p, cell_of = _id_scene(rng, 250, per_cell)
    dp = DataProcessor(_cfg("raw", k=250, shuffle=(True, True)), WAYMO_RANGE, True, 5)
    seeds = 200
    picked = np.zeros(len(p), np.int64)
    pts = torch.from_numpy(p).cuda()
    offs = torch.tensor([0, len(p)], dtype=torch.int64, device="cuda")
    ids = torch.stack([dp((pts, offs, len(p)), seed=s, check=False)["points"][:, 4] for s in range(seeds)]).cpu().numpy().astype(np.int64)
    for row in ids:
        assert np.array_equal(np.sort(cell_of[row]), np.arange(250))             # one point of every cell
        picked[row] += 1
    m = np.array(per_cell)[cell_of % len(per_cell)]
    mean, sd = seeds / m, np.sqrt(seeds * (1 / m) * (1 - 1 / m))
    z = np.abs(picked - mean) / sd
    print("largest deviation: %.2f sigma" % z.max())
    assert z.max() < 6.0


def _device_batch(rng, cells, boxes_per_scene, n_cap):
    parts = [_id_scene(rng, n, (1, 2, 4), 100000 * b)[0] for b, n in enumerate(cells)]
    flat = np.concatenate(parts)
    packed = torch.zeros((len(cells) * n_cap, 5), dtype=torch.float32, device="cuda")
    packed[:len(flat)] = torch.from_numpy(flat).cuda()
    offs = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in parts])]), dtype=torch.int64, device="cuda")
    bx = []
    for m in boxes_per_scene:
        b = np.zeros((m, 8), np.float32)
        b[:, 0:2] = rng.uniform(-60, 60, (m, 2))
        b[:, 3:6] = [4.0, 1.8, 1.6]
        b[:, 6] = rng.uniform(-3, 3, m)
        b[:, 7] = 1
        b[0, 0] = 90.0                                  # one box per scene outside the range
        bx.append(b)
    boxes = torch.from_numpy(np.concatenate(bx)).cuda()
    boffs = torch.tensor(np.concatenate([[0], np.cumsum(boxes_per_scene)]), dtype=torch.int64, device="cuda")
    return packed, offs, boxes, boffs


@pytest.mark.gpu
@pytest.mark.parametrize("sample_type", ["raw", "mean_vfe"])
def test_no_host_read_path(sample_type):
    from pdanet_amd.data_processor import DataProcessor
    n_cap, k = 12000, 4096
    dp = DataProcessor(_cfg(sample_type, k=k, max_voxels=(4500, 4500)), WAYMO_RANGE, True, 5)
    packed, offs, boxes, boffs = _device_batch(np.random.default_rng(11), [5000, 3000], [7, 12], n_cap)
    torch.cuda.synchronize()
    dp((packed, offs, n_cap), (boxes, boffs), max_gt=16, seed=77, check=False)      # loads the kernels
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        bd = dp((packed, offs, n_cap), (boxes, boffs), max_gt=16, seed=77, check=False)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert bd["points"].shape == (2 * k, 6) and bd["gt_boxes"].shape == (2, 16, 8)
    assert bd["voxel_info"][:, 2].tolist() == [5000, 3000] and bd["voxel_info"][:, 3].tolist() == [16, 0]
    assert bd["input_info"][:, 0].tolist() == [4500, 3000] and bd["input_info"][:, 2].tolist() == [6, 11]
    assert (bd["input_info"][:, 3] == 0).all()
    # captured into a graph and replayed on other scenes within n_cap
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = dp((packed, offs, n_cap), (boxes, boffs), max_gt=16, seed=77, check=False)
    g.replay()
    assert torch.equal(static["points"], bd["points"])
    p2, o2, _, _ = _device_batch(np.random.default_rng(12), [2500, 4400], [7, 12], n_cap)
    packed.copy_(p2); offs.copy_(o2)
    g.replay()
    eager = dp((packed, offs, n_cap), (boxes, boffs), max_gt=16, seed=77, check=False)
    torch.cuda.synchronize()
    assert torch.equal(static["points"], eager["points"]) and torch.equal(static["voxel_info"], eager["voxel_info"])
    assert static["voxel_info"][:, 2].tolist() == [2500, 4400]


@pytest.mark.gpu
def test_a_bad_perm0_flags_the_scene():
    from pdanet_amd.data_processor import DataProcessor
    rng = np.random.default_rng(13)
    a, _ = _id_scene(rng, 700, (1, 2))
    b, _ = _id_scene(rng, 500, (1, 3))
    k = 512
    dp = DataProcessor(_cfg("raw", k=k, shuffle=(True, True)), WAYMO_RANGE, True, 5)
    pick, perm1 = [np.arange(k)] * 2, [np.arange(k)] * 2
    good = [rng.permutation(len(a)), rng.permutation(len(b))]
    ok = dp([a, b], draws={"perm0": good, "pick": pick, "perm1": perm1})
    assert (ok["voxel_info"][:, 3] == 0).all()
    out_of_range = good[1].copy()
    out_of_range[out_of_range == 3] = len(b)                         # no duplicate, one entry past the end
    for bad in (good[1][:-1], np.concatenate([good[1], [0]]), out_of_range):
        draws = {"perm0": [good[0], bad], "pick": pick, "perm1": perm1}
        with pytest.raises(ValueError, match="scene 1: perm0"):
            dp([a, b], draws=draws)
        bd = dp([a, b], draws=draws, check=False)
        assert bd["voxel_info"][0, 3].item() == 0 and bd["voxel_info"][1, 3].item() & 8
        assert bd["voxel_info"][1, 2].item() == 0 and bd["input_info"][1, 3].item() & 1       # written empty
        assert torch.equal(bd["points"][:k], ok["points"][:k]) and not bd["points"][k:, 1:].any()
    with pytest.raises(ValueError, match="perm0"):
        dp([a, b], draws={"pick": pick, "perm1": perm1})


# ---- the detector fed from the stage -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_detector_trains_on_voxel_stage_output():
    from pdanet_amd import detector
    from pdanet_amd.data_processor import DataProcessor
    torch.manual_seed(7)
    model, cfg = detector.build_detector("kitti_pda_ssd.yaml")
    model = model.cuda()
    dc = cfg["DATA_CONFIG"]
    rng = np.random.default_rng(21)

    def scene(n):
        p = np.zeros((n, 4), np.float32)
        p[:, 0], p[:, 1] = rng.uniform(2, 68, n), rng.uniform(-38, 38, n)
        p[:, 2], p[:, 3] = rng.uniform(-2.5, 0.5, n), rng.uniform(0, 1, n)
        p[:n // 4, 0] = rng.uniform(-30, -1, n // 4)                 # behind the sensor: outside the range
        return p[rng.permutation(n)]

    def boxes(m):
        b = np.zeros((m, 8), np.float32)
        b[:, 0], b[:, 1], b[:, 2] = rng.uniform(5, 65, m), rng.uniform(-35, 35, m), -1.0
        b[:, 3:6] = [3.9, 1.6, 1.5]
        b[:, 6], b[:, 7] = rng.uniform(-np.pi, np.pi, m), rng.integers(1, 4, m)
        b[0, 0] = -20.0                                               # outside
        return b

    k = 16384
    dp = DataProcessor(_cfg("mean_vfe", k=k, voxel_size=(0.2, 0.2, 0.3), max_voxels=(20000, 20000)), dc["POINT_CLOUD_RANGE"], True,
                       dc["NUM_POINT_FEATURES"])
    bd = dp([scene(40000), scene(24000)], [boxes(7), boxes(12)], max_gt=32, seed=5)
    assert bd["points"].shape == (2 * k, 5) and bd["gt_boxes"].shape == (2, 32, 8)
    assert bd["input_info"][:, 2].tolist() == [6, 11]
    vinfo = bd["voxel_info"].cpu().numpy()
    assert vinfo[:, 0].tolist() == [30000, 18000] and (vinfo[:, 2] > k // 2).all()
    model.train()
    ret, _, _ = model(bd)
    assert torch.isfinite(ret["loss"])
    ret["loss"].backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
