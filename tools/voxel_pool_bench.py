#!/usr/bin/env python
"""Times VoxelRCNNHead.roi_grid_pool at the KITTI training shape of voxel_rcnn_car.yaml: 2 synthetic scenes through
VoxelGenerator at the yaml's voxel size (0.05, 0.05, 0.1 m over [0, -40, -3, 70.4, 40, 1], at most 16000 voxels a scene),
MeanVFE and VoxelBackBone8x for the three sparse levels at realistic voxel counts, 128 car-sized RoIs a scene, grid 6:
M = 2 x 128 x 216 = 55296 grid points, 16 samples each, 32 channels.

Two paths side by side (voxel_pool_modules.py): `fused` (csrc/voxel_pool.hip) and `composed`, the reference's composition
over the stacked grouping operators and torch modules.  One JSON line per (sources, mode, path): the median and the
minimum over --reps calls, wall clock between two device synchronisations, after --warmup calls, the two paths alternating
call by call so that both see the same machine; and the peak of torch.cuda.max_memory_allocated over one call, absolute and
above what was allocated before the call.

  sources   one of x_conv2 / x_conv3 / x_conv4 alone (a head built with that single source), or all three: the head's
            whole roi_grid_pool.
  mode      train_fwd_bwd: training-mode forward and the backward of the sum of squares, into the sparse features and the
            layers' parameters.  eval_fwd: eval-mode forward under no_grad.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdanet_amd import voxel_pool_modules as vpm  # noqa: E402
from pdanet_amd.config import to_attr  # noqa: E402
from pdanet_amd.mean_vfe import MeanVFE  # noqa: E402
from pdanet_amd.spconv_backbone import VoxelBackBone8x  # noqa: E402
from pdanet_amd.voxel_utils import VoxelGenerator, collate_voxels, grid_size  # noqa: E402
from pdanet_amd.voxelrcnn_head import VoxelRCNNHead  # noqa: E402

PCR = [0, -40, -3, 70.4, 40, 1]
VS = [0.05, 0.05, 0.1]
SOURCES = ['x_conv2', 'x_conv3', 'x_conv4']
RADII = {'x_conv2': 0.4, 'x_conv3': 0.8, 'x_conv4': 1.6}


def head_cfg(sources):
    layers = {s: {'MLPS': [[32, 32]], 'QUERY_RANGES': [[4, 4, 4]], 'POOL_RADIUS': [RADII[s]], 'NSAMPLE': [16],
                  'POOL_METHOD': 'max_pool'} for s in sources}
    return {
        'CLASS_AGNOSTIC': True, 'SHARED_FC': [256, 256], 'CLS_FC': [256, 256], 'REG_FC': [256, 256], 'DP_RATIO': 0.3,
        'ROI_GRID_POOL': {'FEATURES_SOURCE': list(sources), 'PRE_MLP': True, 'GRID_SIZE': 6, 'POOL_LAYERS': layers},
        'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5, 'SAMPLE_ROI_BY_EACH_CLASS': True,
                          'CLS_SCORE_TYPE': 'roi_iou', 'CLS_FG_THRESH': 0.75, 'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1,
                          'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55},
        'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                        'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,
                                         'code_weights': [1.0] * 7}},
    }


def scenes(rng, batch, n_points, n_boxes=40):
    """A crude lidar sweep a scene (ground returns thinning with range, upright boxes of returns) and the boxes' centres."""
    pts, centres = [], []
    for _ in range(batch):
        r = np.abs(rng.standard_normal(n_points)) * 22 + 2
        az = rng.uniform(-0.72, 0.72, n_points)
        x, y = r * np.cos(az), r * np.sin(az)
        z = -1.7 + rng.standard_normal(n_points) * 0.03 + 0.002 * r
        k = n_points // 3
        cx, cy = rng.uniform(5, 60, n_boxes), rng.uniform(-30, 30, n_boxes)
        which = rng.integers(0, n_boxes, k)
        x[:k], y[:k] = cx[which] + rng.uniform(-2, 2, k), cy[which] + rng.choice([-0.8, 0.8], k) + rng.standard_normal(k) * 0.02
        z[:k] = rng.uniform(-1.7, 0.2, k)
        pts.append(np.stack([x, y, z, rng.random(n_points)], axis=1).astype(np.float32))
        centres.append(np.stack([cx, cy], axis=1))
    return pts, centres


def rois_for(rng, centres, per_scene):
    """Car-sized proposals: three quarters jittered around the scenes' objects, the rest anywhere in the range."""
    out = np.zeros((len(centres), per_scene, 7), np.float32)
    for b, c in enumerate(centres):
        near = c[rng.integers(0, len(c), per_scene)] + rng.standard_normal((per_scene, 2)) * 0.5
        anywhere = np.stack([rng.uniform(2, 68, per_scene), rng.uniform(-38, 38, per_scene)], axis=1)
        xy = np.where((rng.random(per_scene) < 0.75)[:, None], near, anywhere)
        out[b, :, 0:2] = xy
        out[b, :, 2] = -0.9 + rng.standard_normal(per_scene) * 0.1
        out[b, :, 3:6] = np.array([3.9, 1.6, 1.56]) * (1 + rng.standard_normal((per_scene, 3)) * 0.08)
        out[b, :, 6] = rng.uniform(-np.pi, np.pi, per_scene)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--points', type=int, default=60000)
    ap.add_argument('--rois', type=int, default=128)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("voxel_pool_bench needs the GPU: there is no CPU path to time")
    rng = np.random.default_rng(0)
    pts, centres = scenes(rng, args.batch, args.points)
    packed = torch.from_numpy(np.concatenate(pts)).cuda()
    offs = torch.tensor(np.cumsum([0] + [len(p) for p in pts]), dtype=torch.int64).cuda()
    voxels, coords, num = collate_voxels(*VoxelGenerator(VS, PCR, 4, 5, 16000).generate_batch((packed, offs, args.points)))
    grid = grid_size(np.array(PCR, np.float64), np.array(VS)).tolist()
    feats = MeanVFE({}, 4)({'voxels': voxels, 'voxel_num_points': num})['voxel_features']
    torch.manual_seed(0)
    backbone = VoxelBackBone8x(to_attr({}), 4, grid).cuda().eval()
    with torch.no_grad():
        bb = backbone({'voxel_features': feats, 'voxel_coords': coords, 'batch_size': args.batch})
    levels = bb['multi_scale_3d_features']
    rois = torch.from_numpy(rois_for(rng, centres, args.rois)).cuda()
    m = args.batch * args.rois * 216
    lines = [dict(stage='input', batch=args.batch, rois_per_scene=args.rois, grid_points=m, voxels=int(coords.shape[0]),
                  level_rows={s: int(levels[s].features.shape[0]) for s in SOURCES},
                  dense_map_bytes={s: int(args.batch * np.prod(levels[s].spatial_shape) * 4) for s in SOURCES})]

    def batch_dict(requires_grad):
        f = {s: levels[s].replace_feature(levels[s].features.detach().clone().requires_grad_(requires_grad)) for s in SOURCES}
        return {'batch_size': args.batch, 'rois': rois, 'multi_scale_3d_features': f,
                'multi_scale_3d_strides': bb['multi_scale_3d_strides']}

    for sources in [[s] for s in SOURCES] + [SOURCES]:
        torch.manual_seed(1)
        head = VoxelRCNNHead(backbone.backbone_channels, to_attr(head_cfg(sources)), PCR, VS, 1).cuda()

        def train_call():
            head.train()
            for prm in head.parameters():
                prm.grad = None
            (head.roi_grid_pool(batch_dict(True)) ** 2).sum().backward()

        def eval_call():
            head.eval()
            with torch.no_grad():
                head.roi_grid_pool(batch_dict(False))

        def on(path, fn):
            def run():
                os.environ[vpm.ENV] = path
                fn()
            return run

        for mode, fn in (('train_fwd_bwd', train_call), ('eval_fwd', eval_call)):
            variants = {'fused': on('fused', fn), 'composed': on('composed', fn)}
            times = {k: [] for k in variants}
            for it in range(args.warmup + args.reps):
                for name, run in variants.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run()
                    torch.cuda.synchronize()
                    if it >= args.warmup:
                        times[name].append((time.perf_counter() - t0) * 1e3)
            for name, run in variants.items():
                for prm in head.parameters():
                    prm.grad = None
                torch.cuda.synchronize()
                before = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                run()
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated()
                lines.append(dict(stage='roi_grid_pool', sources="+".join(sources), mode=mode, path=name,
                                  median_ms=float(np.median(times[name])), min_ms=float(np.min(times[name])),
                                  peak_bytes=int(peak), peak_above_start_bytes=int(peak - before)))
        os.environ.pop(vpm.ENV, None)

    text = "\n".join(json.dumps(line) for line in lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
