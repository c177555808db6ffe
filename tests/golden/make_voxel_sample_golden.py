#!/usr/bin/env python
"""Generates tests/golden/voxel_sample.npz: the REFERENCE's voxel down-sampling chain
(pcdet/datasets/processor/data_processor.py DataProcessor: mask_points_and_boxes_outside_range ->
shuffle_points -> sample_points_by_voxels, then pcdet/datasets/dataset.py DatasetTemplate.collate_batch) run on synthetic
ragged scenes, with every draw it makes recorded as make_input_golden.py records them; np.random.permutation is the LEADING
shuffle here and is stored as `perm0`.

spconv / cumm are not installed, so VoxelGeneratorWrapper is replaced by PyVoxelGenerator below: a plain-Python restatement
of the CPU loop of spconv's point-to-voxel (Point2VoxelCPU3d.point_to_voxel / VoxelGeneratorV2), float32 arithmetic through
numpy scalars.  spconv itself was not run.  Everything else -- the mask, the shuffle, the raw / mean_vfe reduction, sample_points,
collate_batch -- is the reference's own code.  Only inputs, draws and outputs are stored.

Two sets of scenes: `raw` holds points within 2e-5 m of the 40 m sphere that sample_points tests; `mean` does not, and the
generator asserts that no voxel mean lies within 1e-4 m of the sphere (the reference tests the float64 means in float64, the
device the float32 rows in float32).

Run with the reference checkout:  python tests/golden/make_voxel_sample_golden.py /path/to/reference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_input_golden as mig   # noqa: E402  (the scene helpers, the draw recorder, its loading of the processor)
from reference_loader import q, reference_root  # noqa: E402
from pdanet_amd.config import AttrDict as AD  # noqa: E402

OUT = os.path.join(HERE, "voxel_sample.npz")
K = 2048
C = 5
RANGE = [-51.2, -51.2, -3.0, 51.2, 51.2, 2.0]
VOXEL_SIZE = [0.4, 0.4, 0.5]
MAX_POINTS = 5
MAX_VOXELS = {"train": 3000, "test": 3200}
COUNTS = []          # per generate() call: [n_points, n_in_grid, n_voxels_before_cap]


class PyVoxelGenerator:
    """VoxelGeneratorWrapper's interface around the loop of spconv's CPU point-to-voxel."""

    def __init__(self, vsize_xyz, coors_range_xyz, num_point_features, max_num_points_per_voxel, max_num_voxels):
        self.vs = np.asarray(vsize_xyz, np.float32)
        self.lo = np.asarray(coors_range_xyz, np.float32)[:3]
        rng = np.asarray(coors_range_xyz, np.float32)
        self.grid = np.round((rng[3:6] - rng[0:3]) / np.array(vsize_xyz)).astype(np.int64)
        self.c, self.max_points, self.max_voxels = num_point_features, max_num_points_per_voxel, max_num_voxels

    def generate(self, points):
        assert points.dtype == np.float32 and points.shape[1] == self.c
        voxels = np.zeros((self.max_voxels, self.max_points, self.c), np.float32)
        coords = np.zeros((self.max_voxels, 3), np.int32)
        num = np.zeros((self.max_voxels,), np.int32)
        index, voxel_num, in_grid, cells = {}, 0, 0, set()
        for i in range(points.shape[0]):
            cell, ok = [0, 0, 0], True
            for j in range(3):
                f = np.floor((points[i, j] - self.lo[j]) / self.vs[j])          # float32 scalars: float32 arithmetic
                assert f.dtype == np.float32
                if not (f >= 0 and f < self.grid[j]):
                    ok = False
                    break
                cell[2 - j] = int(f)
            if not ok:
                continue
            in_grid += 1
            cell = tuple(cell)
            cells.add(cell)
            v = index.get(cell)
            if v is None:
                if voxel_num >= self.max_voxels:
                    continue
                v = voxel_num
                voxel_num += 1
                index[cell] = v
                coords[v] = cell
            if num[v] < self.max_points:
                voxels[v, num[v]] = points[i]
                num[v] += 1
        COUNTS.append([points.shape[0], in_grid, len(cells)])
        return voxels[:voxel_num], coords[:voxel_num], num[:voxel_num]


# ---- synthetic scenes ----------------------------------------------------------------------------------------------------
def _cells(rng, n_cells, rmin, rmax, per_cell):
    """Points of n_cells distinct cells whose centres lie at horizontal distance [rmin, rmax): per_cell(rng) points each,
    at least 0.03 m inside the cell, coordinates on a 1/256 grid."""
    lo, vs = np.array(RANGE[:3]), np.array(VOXEL_SIZE)
    grid = np.round((np.array(RANGE[3:]) - lo) / vs).astype(int)
    seen, rows = set(), []
    while len(seen) < n_cells:
        r, a = np.sqrt(rng.uniform(rmin ** 2, rmax ** 2)), rng.uniform(-np.pi, np.pi)
        cell = (int((r * np.cos(a) - lo[0]) // vs[0]), int((r * np.sin(a) - lo[1]) // vs[1]), int(rng.integers(1, grid[2] - 1)))
        ctr = lo + (np.array(cell) + 0.5) * vs
        d = np.hypot(ctr[0], ctr[1])
        if cell in seen or not (0 < cell[0] < grid[0] - 1 and 0 < cell[1] < grid[1] - 1) or not (rmin + 0.5 <= d < rmax - 0.5):
            continue
        seen.add(cell)
        m = per_cell(rng)
        p = np.zeros((m, C), np.float32)
        p[:, :3] = q(lo + (np.array(cell) + rng.uniform(0.1, 0.9, (m, 3))) * vs)
        p[:, 3:] = q(rng.uniform(0, 1, (m, C - 3)))
        rows.append(p)
    return np.concatenate(rows)


def _faces():
    """Points exactly on voxel faces (float32(lo + k * vs)) and one float step either side, per axis; x == xmax, y == ymax,
    z below and above the range."""
    f = np.float32
    lo, vs = np.array(RANGE[:3]), np.array(VOXEL_SIZE)
    mid = [f(3.3), f(-7.1), f(-0.8)]
    rows = []
    for axis, ks in ((0, (1, 37, 130, 201, 255)), (1, (2, 64, 99, 177, 254)), (2, (1, 3, 4, 7, 9))):
        for k in ks:
            face = f(lo[axis] + k * vs[axis])
            for v in (face, np.nextafter(face, f(-1e9)), np.nextafter(face, f(1e9))):
                p = list(mid)
                p[axis] = v
                p[(axis + 1) % 3] = f(p[(axis + 1) % 3] + 0.4 * (k % 7))       # spread over several cells
                rows.append(p)
    rows += [[f(RANGE[3]), mid[1], mid[2]], [mid[0], f(RANGE[4]), mid[2]], [f(RANGE[0]), f(RANGE[1]), mid[2]],
             [mid[0], mid[1], f(RANGE[2] - 0.7)], [mid[0], mid[1], f(RANGE[5] + 0.7)], [mid[0], mid[1], f(RANGE[5])]]
    p = np.zeros((len(rows), C), np.float32)
    p[:, :3] = np.array(rows, np.float32)
    p[:, 3:] = f(0.5)
    return p


def make_scenes(rng, with_sphere):
    few = lambda r: int(r.choice([1, 1, 1, 1, 2, 5, 6]))                  # noqa: E731  1, exactly 5 and more than 5 points
    one = lambda r: int(r.choice([1, 1, 1, 1, 2]))                        # noqa: E731
    many = lambda r: int(r.choice([1, 2, 3, 5, 6, 8]))                    # noqa: E731
    s = []
    # case A: more voxels than K, fewer than K of them far; the face points; points on the 40 m sphere (raw only)
    a = [_cells(rng, 1500, 2, 39, few), _cells(rng, 650, 41, 50, one), _faces(), mig._outside(rng, 150, RANGE, C)]
    if with_sphere:
        a.append(mig._sphere(rng, 250, C, False))
    s.append(np.concatenate(a))
    # case B, capped: more occupied voxels than MAX_NUMBER_OF_VOXELS, at least K far voxels among the kept ones
    s.append(np.concatenate([_cells(rng, 500, 2, 39, one), _cells(rng, 3100, 41, 50, one), mig._outside(rng, 100, RANGE, C)]))
    # case C: fewer voxels than K
    s.append(np.concatenate([_cells(rng, 700, 2, 39, many), _cells(rng, 300, 41, 50, many), mig._outside(rng, 300, RANGE, C)]))
    boxes = [mig._boxes(rng, 8, RANGE, "mixed"), mig._boxes(rng, 5, RANGE, "mixed"), mig._boxes(rng, 4, RANGE, "outside")]
    return s, boxes


def run(DataProcessor, collate, scenes, boxes, sample_type, training):
    cfg = [AD(NAME="mask_points_and_boxes_outside_range", REMOVE_OUTSIDE_BOXES=True),
           AD(NAME="shuffle_points", SHUFFLE_ENABLED=AD(train=True, test=False)),
           AD(NAME="sample_points_by_voxels", SAMPLE_TYPE=sample_type, VOXEL_SIZE=VOXEL_SIZE, MAX_POINTS_PER_VOXEL=MAX_POINTS,
              MAX_NUMBER_OF_VOXELS=AD(MAX_VOXELS), NUM_POINTS=AD(train=K, test=K))]
    dp = DataProcessor(cfg, np.array(RANGE, np.float32), training, C)
    rec = mig.Recorder()
    outs, draws, cases = [], {"pick": [], "perm1": [], "perm0": []}, []
    del COUNTS[:]
    with rec:
        for pts, bx in zip(scenes, boxes):
            rec.reset()
            dp.voxel_generator = None                      # a fresh generator per scene, as the loop is stateless anyway
            d = dp.forward({"points": pts.copy(), "gt_boxes": bx.copy(), "use_lead_xyz": True})
            d.pop("use_lead_xyz")
            outs.append(d)
            draws["pick"].append(rec.pick)
            draws["perm1"].append(rec.perm1)
            draws["perm0"].append(rec.perm2 if training else np.zeros(0, np.int32))     # Recorder names permutation() perm2
    batch = collate(outs)
    return batch, draws, np.array(COUNTS, np.int32)


def voxel_rows(points, training, perm0, sample_type):
    """The rows sample_points sees, recomputed here only for the generator's own assertions and case report."""
    rng6 = np.array(RANGE, np.float32)
    m = (points[:, 0] >= rng6[0]) & (points[:, 0] <= rng6[3]) & (points[:, 1] >= rng6[1]) & (points[:, 1] <= rng6[4])
    p = points[m]
    if training:
        p = p[perm0]
    vox, _, num = PyVoxelGenerator(VOXEL_SIZE, rng6, C, MAX_POINTS, MAX_VOXELS["train" if training else "test"]).generate(p)
    COUNTS.pop()
    if sample_type == "mean_vfe":
        return vox.sum(axis=1) / np.expand_dims(num, 1).repeat(C, axis=-1), num
    return vox[:, 0], num


def main():
    DataProcessor, collate = mig.import_reference(reference_root())
    sys.modules["pcdet.datasets.processor.data_processor"].VoxelGeneratorWrapper = PyVoxelGenerator
    rng = np.random.default_rng(20261017)
    data = {"num_points": np.array(K), "range": np.array(RANGE, np.float32), "voxel_size": np.array(VOXEL_SIZE, np.float64),
            "max_points": np.array(MAX_POINTS), "max_voxels": np.array([MAX_VOXELS["train"], MAX_VOXELS["test"]])}
    np.random.seed(17)
    for tag, sample_type in (("raw", "raw"), ("mean", "mean_vfe")):
        scenes, boxes = make_scenes(rng, with_sphere=(tag == "raw"))
        scenes = [s[np.random.permutation(len(s))] for s in scenes]         # scenes arrive in sensor order
        data[tag + "_points_raw"] = np.concatenate(scenes)
        data[tag + "_offsets"] = np.concatenate([[0], np.cumsum([len(s) for s in scenes])]).astype(np.int64)
        data[tag + "_boxes_raw"] = np.concatenate(boxes)
        data[tag + "_box_offsets"] = np.concatenate([[0], np.cumsum([len(b) for b in boxes])]).astype(np.int64)
        for mode in ("train", "test"):
            training = mode == "train"
            batch, draws, counts = run(DataProcessor, collate, scenes, boxes, sample_type, training)
            key = "%s_%s_" % (tag, mode)
            for name in ("pick", "perm1", "perm0"):
                data[key + name] = np.concatenate(draws[name]).astype(np.int32)
                data[key + name + "_offsets"] = np.concatenate([[0], np.cumsum([len(x) for x in draws[name]])]).astype(np.int64)
            data[key + "ref_points"] = batch["points"].astype(np.float32)
            data[key + "ref_gt_boxes"] = batch["gt_boxes"].astype(np.float32)
            data[key + "ref_kept"] = np.array([int((np.abs(batch["gt_boxes"][b]).sum(1) > 0).sum()) for b in range(len(scenes))],
                                              np.int32)
            data[key + "ref_counts"] = counts                       # [n_masked, n_in_grid, n_voxels_before_cap] per scene
            for b, s in enumerate(scenes):
                rows, num = voxel_rows(s, training, draws["perm0"][b], sample_type)
                d = np.linalg.norm(rows[:, :3].astype(np.float64), axis=1)
                if sample_type == "mean_vfe":
                    assert np.abs(d - 40.0).min() > 1e-4, "a voxel mean lies within 1e-4 m of the 40 m sphere"
                n, n_far = len(rows), int((d >= 40.0).sum())
                case = "C" if n <= K else "A" if n_far < K else "B"
                cap = MAX_VOXELS[mode]
                print("%s %s scene %d: %d raw points, counts %s, %d voxels (cap %d%s), %d far -> case %s; voxels with 1 "
                      "point: %d, full: %d; rows within 2e-5 m of the sphere: %d"
                      % (tag, mode, b, len(s), counts[b].tolist(), n, cap, ", HIT" if counts[b][2] > cap else "", n_far, case,
                         int((num == 1).sum()), int((num == MAX_POINTS).sum()), int((np.abs(d - 40.0) < 2e-5).sum())))
    np.savez_compressed(OUT, **data)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
