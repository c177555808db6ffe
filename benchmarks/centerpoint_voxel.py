#!/usr/bin/env python
"""Times voxel CenterPoint's padded training iteration (forward + loss + backward) at kitti_models/centerpoint.yaml's model --
MeanVFE, VoxelResBackBone8x, HeightCompression, BaseBEVBackbone, CenterHead over 3 classes -- on KITTI's grid (range
[0, -40, -3, 70.4, 40, 1], voxels 0.05 x 0.05 x 0.1: 1408 x 1600 x 40, at most 16000 voxels of 5 points a scene) and the
synthetic voxels of benchmarks/second_padded.py, with the residual tails of the backbone's eight SparseBasicBlocks two ways:

  fused      PDA_RES_BN unset: relu(bn2(x) + identity) in one counted kernel pair (pda_bn_add_relu_*_counted);
  composed   PDA_RES_BN=composed: the counted BatchNorm, `+` and ReLU as three steps (what the fused pair replaces),

each eager and replayed from its own captured graph.  The four sides alternate inside one process; every figure is a
wall-clock time between two device synchronisations per call, `--steps` calls after `--warmup` calls, in milliseconds: median,
minimum, maximum.  The losses of the sides are compared before anything is timed (fused and composed give the same bits).
PADDED_CAPS = the level counts of the same data + 25 %, taken from one compact iteration.  A measurement, not a gate:
prints one JSON line.

    python benchmarks/centerpoint_voxel.py [--steps 20] [--warmup 5] [--voxels 12000,9000,14000,10000]
"""
import argparse
import gc
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "benchmarks")]

from pdanet_amd import spconv_utils                                                                    # noqa: E402
from pdanet_amd.centerpoint import build                                                               # noqa: E402
from pdanet_amd.config import to_attr                                                                  # noqa: E402
from anchor_head_bench import synth                                                                    # noqa: E402
from second_padded import LEVELS, MAX_VOXELS, PCR, VOXEL, synthetic_voxels, timed_alternating          # noqa: E402

SWITCH = "PDA_RES_BN"


def model_cfg():
    with open(os.path.join(ROOT, "tests", "golden", "centerpoint_voxel_state_dict.json")) as f:
        return json.load(f)['kitti']['config']['MODEL']          # centerpoint.yaml's MODEL block as it is


def set_mode(mode):
    if mode == "fused":
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = mode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--voxels", default="12000,9000,14000,10000", help="live voxels per scene (at most %d each)" % MAX_VOXELS)
    ap.add_argument("--max-gt", type=int, default=48)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/centerpoint_voxel.py needs the GPU: a CPU run gives no time")
    torch.cuda.set_device(0)
    live = [int(v) for v in args.voxels.split(",")]
    B = len(live)
    assert all(0 < n <= MAX_VOXELS for n in live)
    pcr, vs = np.array(PCR, np.float64), np.array(VOXEL, np.float64)
    grid = np.round((pcr[3:] - pcr[:3]) / vs).astype(np.int64)
    dataset = {'class_names': ['Car', 'Pedestrian', 'Cyclist'], 'point_cloud_range': PCR, 'voxel_size': VOXEL, 'num_point_features': 4}
    torch.manual_seed(0)
    model = build(to_attr(model_cfg()), 3, dataset).cuda().train()
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
        last['out'] = batch['encoded_spconv_tensor']
        return (ret['loss'].detach(),) + torch.autograd.grad(ret['loss'], params)

    def forget():
        last.clear()
        model.dense_head.forward_ret_dict.clear()

    step(compact)                                                          # the level counts of this data
    counts = {k: last['out'].indice_dict[k].n_out for k in list(LEVELS) + ['spconv_down2']}
    model.backbone_3d.model_cfg = to_attr({'PADDED_CAPS': {k: int(np.ceil(n * 1.25)) for k, n in counts.items()}})
    forget()
    losses, graphs, kept = {}, {}, []
    for mode in ("fused", "composed"):
        set_mode(mode)
        out = step(padded)
        losses[mode] = float(out[0])
        live_rows, cap_rows, status = spconv_utils.padded_report(last['out'])
        del out
        forget()
        # one graph of this side: nothing of an earlier iteration alive at the capture (DESIGN.md "Known gaps")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(padded)
        torch.cuda.current_stream().wait_stream(side)
        forget()
        gc.collect()
        torch.cuda.synchronize()
        graphs[mode] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[mode]):
            kept.append(step(padded))
        forget()
        graphs[mode].replay()
        torch.cuda.synchronize()
        losses[mode + "_graph"] = float(kept[-1][0])
    result = {"benchmark": "centerpoint_voxel", "batch": B, "grid": grid.tolist(), "live_voxels": live, "capacity": cap,
              "steps": args.steps, "warmup": args.warmup, "unit": "wall-clock ms per iteration (median, min, max)",
              "device": torch.cuda.get_device_name(0), "loss": losses, "status": status, "live_rows": live_rows,
              "cap_rows": cap_rows}

    def eager(mode):
        def run():
            set_mode(mode)
            step(padded)
            forget()
        return run

    result["iteration"] = timed_alternating({"fused": eager("fused"), "composed": eager("composed"),
                                             "fused_graph": graphs["fused"].replay, "composed_graph": graphs["composed"].replay},
                                            args.steps, args.warmup)
    it = result["iteration"]
    result["fused_over_composed"] = {"eager": round(it["fused"][0] / it["composed"][0], 4),
                                     "graph": round(it["fused_graph"][0] / it["composed_graph"][0], 4)}
    result["status_after"] = padded['voxel_status'].tolist()[0]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
