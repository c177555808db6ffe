#!/usr/bin/env python
"""Times StackSAModuleMSG, forward + backward, at two shapes of kitti_models/pv_rcnn.yaml with 2 synthetic scenes:

  roi_grid   PVRCNNHead's RoI-grid pool at the training shape: N = 2 x 2048 keypoints with 128 channels, M = 2 x 128 x 216 =
             55296 grid points of car-sized RoIs, two scales 128 -> 64 -> 64, nsample 16 / 16, radii 0.8 / 1.6.
  x_conv3    VoxelSetAbstraction's layer over the third sparse level: the occupied cells of the stride-4 grid (0.2, 0.2, 0.4 m)
             under a synthetic sweep with 64 channels, M = 2 x 2048 keypoints, two scales 64 -> 64 -> 64, nsample 16 / 32,
             radii 1.2 / 2.4.

Two paths side by side (pointnet2_stack_modules.py): `fused` (csrc/stack_sa.hip) and `composed`, the reference's operator
sequence over the stacked ball query / grouping kernels and torch modules.  One JSON line per (shape, mode, path): the median
and the minimum over --reps calls, wall clock between two device synchronisations, after --warmup calls, the two paths
alternating call by call so that both see the same machine; and the peak of torch.cuda.max_memory_allocated over one call,
absolute and above what was allocated before the call (the inputs and the parameters).

  mode      train_fwd_bwd: training-mode forward and the backward of the sum of squares, into the features and the layer's
            parameters.  eval_fwd: eval-mode forward under no_grad.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from pdanet_amd import pointnet2_stack_modules as psm  # noqa: E402
from pdanet_amd.pvrcnn_head import PVRCNNHead  # noqa: E402
from voxel_pool_bench import PCR, rois_for, scenes  # noqa: E402


def roi_grid_shape(rng, pts, centres, rois_per_scene, keypoints):
    """keypoints drawn from the sweep, the grid points of the RoIs -> xyz, its counts, new_xyz, its counts"""
    xyz = np.concatenate([p[rng.choice(len(p), keypoints, replace=False), :3] for p in pts]).astype(np.float32)
    rois = torch.from_numpy(rois_for(rng, centres, rois_per_scene))
    grid, _ = PVRCNNHead.get_global_grid_points_of_roi(PVRCNNHead, rois, 6)
    new_xyz = grid.reshape(-1, 3).contiguous()
    return (torch.from_numpy(xyz), torch.full((len(pts),), keypoints, dtype=torch.int32), new_xyz,
            torch.full((len(pts),), rois_per_scene * 216, dtype=torch.int32))


def level_shape(rng, pts, keypoints, cell=(0.2, 0.2, 0.4)):
    """the centres of the occupied cells of a coarse grid, keypoints drawn from the sweep"""
    lo, cell = np.array(PCR[:3], np.float32), np.array(cell, np.float32)
    xyz, cnt, new_xyz = [], [], []
    for p in pts:
        inside = p[((p[:, :3] >= lo) & (p[:, :3] < np.array(PCR[3:], np.float32))).all(axis=1)]
        cells = np.unique(np.floor((inside[:, :3] - lo) / cell).astype(np.int64), axis=0)
        xyz.append(((cells + 0.5) * cell + lo).astype(np.float32))
        cnt.append(len(cells))
        new_xyz.append(inside[rng.choice(len(inside), keypoints, replace=False), :3])
    return (torch.from_numpy(np.concatenate(xyz)), torch.tensor(cnt, dtype=torch.int32), torch.from_numpy(np.concatenate(new_xyz)),
            torch.full((len(pts),), keypoints, dtype=torch.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--points', type=int, default=60000)
    ap.add_argument('--rois', type=int, default=128)
    ap.add_argument('--keypoints', type=int, default=2048)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stack_sa_bench needs the GPU: there is no CPU path to time")
    rng = np.random.default_rng(0)
    pts, centres = scenes(rng, args.batch, args.points)
    shapes = {
        'roi_grid': (roi_grid_shape(rng, pts, centres, args.rois, args.keypoints), 128,
                     dict(radii=[0.8, 1.6], nsamples=[16, 16], mlps=[[128, 64, 64], [128, 64, 64]])),
        'x_conv3': (level_shape(rng, pts, args.keypoints), 64,
                    dict(radii=[1.2, 2.4], nsamples=[16, 32], mlps=[[64, 64, 64], [64, 64, 64]])),
    }
    lines = []
    for name, (geometry, c_in, spec) in shapes.items():
        xyz, cnt, new_xyz, new_cnt = (t.cuda() for t in geometry)
        feat = torch.randn(xyz.shape[0], c_in, generator=torch.Generator().manual_seed(1)).cuda()
        torch.manual_seed(1)
        mod = psm.StackSAModuleMSG(use_xyz=True, pool_method='max_pool', **spec).cuda()
        assert all(mod.is_fused(k) for k in range(2))
        lines.append(dict(stage='input', shape=name, source_rows=int(xyz.shape[0]), centres=int(new_xyz.shape[0]), c_in=c_in, **spec))

        def train_call():
            mod.train()
            for prm in mod.parameters():
                prm.grad = None
            f = feat.detach().requires_grad_(True)
            (mod(xyz, cnt, new_xyz, new_cnt, f)[1] ** 2).sum().backward()

        def eval_call():
            mod.eval()
            with torch.no_grad():
                mod(xyz, cnt, new_xyz, new_cnt, feat)

        def on(path, fn):
            def run():
                os.environ[psm.ENV] = path
                fn()
            return run

        for mode, fn in (('train_fwd_bwd', train_call), ('eval_fwd', eval_call)):
            variants = {'fused': on('fused', fn), 'composed': on('composed', fn)}
            times = {k: [] for k in variants}
            for it in range(args.warmup + args.reps):
                for path, run in variants.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run()
                    torch.cuda.synchronize()
                    if it >= args.warmup:
                        times[path].append((time.perf_counter() - t0) * 1e3)
            for path, run in variants.items():
                for prm in mod.parameters():
                    prm.grad = None
                torch.cuda.synchronize()
                before = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                run()
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated()
                lines.append(dict(stage='stack_sa', shape=name, mode=mode, path=path, median_ms=float(np.median(times[path])),
                                  min_ms=float(np.min(times[path])), peak_bytes=int(peak), peak_above_start_bytes=int(peak - before)))
        os.environ.pop(psm.ENV, None)

    text = "\n".join(json.dumps(line) for line in lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
