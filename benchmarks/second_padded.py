#!/usr/bin/env python
"""Times SECOND's training iteration (forward + loss + backward) at kitti_models/second.yaml's shape -- range
[0, -40, -3, 70.4, 40, 1], voxels 0.05 x 0.05 x 0.1 (grid 1408 x 1600 x 40), MeanVFE, VoxelBackBone8x, BaseBEVBackbone,
AnchorHeadSingle over 3 classes, at most 16000 voxels of 5 points a scene -- on synthetic voxels, three ways:

  compact        today's path: the voxels cut to the live rows, one host read per strided convolution (four an iteration);
  padded         the read-free form: all batch * 16000 rows, voxel_num_active on the device, counted
                 BatchNorm, PADDED_CAPS = the level counts of the same data + 25 %;
  padded_graph   the same iteration captured once and replayed.

The voxel collate is outside all three (the compact collate reads the host once more).  The sides alternate inside one
process; every figure is a wall-clock time between two device synchronisations per call (the compact side reads the host,
so device events alone would not see its waits), `--steps` calls after `--warmup` calls, in milliseconds: median, minimum,
maximum.  The losses of the three sides are compared before anything is timed.  A measurement, not a gate: prints one JSON
line.

    python benchmarks/second_padded.py [--steps 20] [--warmup 5] [--voxels 12000,9000,14000,10000]
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from pdanet_amd import spconv_utils                                                                    # noqa: E402
from pdanet_amd.config import to_attr                                                                  # noqa: E402
from pdanet_amd.second_net import SECONDNet                                                            # noqa: E402
from anchor_head_bench import synth                                                                    # noqa: E402

PCR, VOXEL, MAX_VOXELS, MAX_POINTS = [0, -40, -3, 70.4, 40, 1], [0.05, 0.05, 0.1], 16000, 5
LEVELS = {'spconv2': 'x_conv2', 'spconv3': 'x_conv3', 'spconv4': 'x_conv4'}


def model_cfg():
    with open(os.path.join(ROOT, "tests", "golden", "second_state_dict.json")) as f:
        cfg = json.load(f)['config']['MODEL']          # second.yaml's modules; only the range differs from the yaml
    return cfg


def synthetic_voxels(rng, live, grid):
    """Per scene `live` distinct cells, denser near the sensor and in the lower half of the range: (voxels, coords (b, z, y, x),
    num_points) compact, scene after scene."""
    nx, ny, nz = (int(v) for v in grid)
    vox, crd, num = [], [], []
    for b, n in enumerate(live):
        x = np.minimum((rng.random(4 * n) ** 1.7 * nx).astype(np.int64), nx - 1)
        y = rng.integers(0, ny, 4 * n)
        z = np.minimum((rng.random(4 * n) ** 2 * nz * 0.6).astype(np.int64), nz - 1)
        cells = np.unique((z * ny + y) * nx + x)
        cells = rng.permutation(cells)[:n]
        assert len(cells) == n
        crd.append(np.stack([np.full(n, b), cells // (ny * nx), (cells // nx) % ny, cells % nx], axis=1))
        pts = rng.integers(1, MAX_POINTS + 1, n)
        v = rng.standard_normal((n, MAX_POINTS, 4)).astype(np.float32)
        v *= (np.arange(MAX_POINTS)[None, :] < pts[:, None])[..., None]
        vox.append(v)
        num.append(pts)
    return np.concatenate(vox), np.concatenate(crd).astype(np.int32), np.concatenate(num).astype(np.int32)


def timed_alternating(fns, steps, warmup):
    """name -> [median, min, max] wall-clock ms per call between two device synchronisations; the sides take turns."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)] for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--voxels", default="12000,9000,14000,10000", help="live voxels per scene (at most %d each)" % MAX_VOXELS)
    ap.add_argument("--max-gt", type=int, default=48)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/second_padded.py needs the GPU: a CPU run gives no time")
    torch.cuda.set_device(0)
    live = [int(v) for v in args.voxels.split(",")]
    B = len(live)
    assert all(0 < n <= MAX_VOXELS for n in live)
    pcr, vs = np.array(PCR, np.float64), np.array(VOXEL, np.float64)
    grid = np.round((pcr[3:] - pcr[:3]) / vs).astype(np.int64)
    dataset = {'class_names': ['Car', 'Pedestrian', 'Cyclist'], 'point_cloud_range': PCR, 'voxel_size': VOXEL, 'num_point_features': 4}
    torch.manual_seed(0)
    model = SECONDNet(to_attr(model_cfg()), 3, dataset).cuda().train()
    params = list(model.parameters())
    rng = np.random.default_rng(0)
    vox, crd, num = synthetic_voxels(rng, live, grid)
    gt = torch.from_numpy(synth(rng, B, args.max_gt, ([args.max_gt, 20, 33, 8] * B)[:B])).cuda()
    dev = lambda a: torch.from_numpy(a).cuda()
    compact = {'voxels': dev(vox), 'voxel_coords': dev(crd), 'voxel_num_points': dev(num), 'gt_boxes': gt, 'batch_size': B}
    total, cap = len(crd), B * MAX_VOXELS
    pad = lambda a, fill: np.concatenate([a, np.full((cap - total,) + a.shape[1:], fill, a.dtype)])
    padded = {'voxels': dev(pad(vox, 0)), 'voxel_coords': dev(pad(crd, -1)), 'voxel_num_points': dev(pad(num, 0)), 'gt_boxes': gt,
              'batch_size': B, 'voxel_num_active': torch.tensor([total], dtype=torch.int32).cuda(),
              'voxel_status': torch.zeros(1, dtype=torch.int32).cuda()}
    last = {}

    def step(batch):
        batch = dict(batch)
        ret, tb, disp = model(batch)
        last['out'] = batch['encoded_spconv_tensor'] if 'voxel_num_active' in batch else None
        counts = {k: batch['multi_scale_3d_features'][v].features.shape[0] for k, v in LEVELS.items()}
        counts['spconv_down2'] = batch['encoded_spconv_tensor'].features.shape[0]
        return (ret['loss'].detach(),) + torch.autograd.grad(ret['loss'], params), counts

    out, counts = step(compact)                                            # the level counts of this data
    loss_compact = float(out[0])
    caps = {k: int(np.ceil(n * 1.25)) for k, n in counts.items()}
    model.backbone_3d.model_cfg = to_attr({'PADDED_CAPS': caps})
    out, _ = step(padded)
    loss_padded = float(out[0])
    live_rows, cap_rows, status = spconv_utils.padded_report(last['out'])
    del out
    last.clear()
    # one graph of the padded iteration: nothing of an earlier iteration alive at the capture (DESIGN.md "Known gaps")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(padded)
    torch.cuda.current_stream().wait_stream(side)
    model.dense_head.forward_ret_dict.clear()
    last.clear()
    gc.collect()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured, _ = step(padded)
    last.clear()
    graph.replay()
    torch.cuda.synchronize()
    result = {"benchmark": "second_padded", "batch": B, "grid": grid.tolist(), "live_voxels": live, "capacity": cap,
              "steps": args.steps, "warmup": args.warmup, "unit": "wall-clock ms per iteration (median, min, max)",
              "device": torch.cuda.get_device_name(0), "loss_compact_padded_graph": [loss_compact, loss_padded, float(captured[0])],
              "status": status, "live_rows": live_rows, "cap_rows": cap_rows,
              "live_over_cap": {k: round(live_rows[k] / max(cap_rows[k], 1), 4) for k in live_rows}}

    def run_compact():
        step(compact)
        model.dense_head.forward_ret_dict.clear()

    def run_padded():
        step(padded)
        last.clear()
        model.dense_head.forward_ret_dict.clear()

    result["iteration"] = timed_alternating({"compact": run_compact, "padded": run_padded, "padded_graph": graph.replay},
                                            args.steps, args.warmup)
    result["status_after"] = padded['voxel_status'].tolist()[0]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
