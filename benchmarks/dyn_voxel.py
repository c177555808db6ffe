#!/usr/bin/env python
"""Times dynamic voxelization at the size the Waymo recipes run it: 8 scenes x 180 000 points, C = 5, in the voxel setting of
voxel_rcnn_with_centerhead_dyn_voxel.yaml and the pillar setting of centerpoint_dyn_pillar_1x.yaml.

Per setting: the index stage alone (dyn_voxel_utils.dynamic_voxel_index) and the encoder's whole forward (DynamicMeanVFE /
DynamicPillarVFE, train-mode BatchNorm, no autograd graph), each next to the composition a user without torch_scatter would
write on the same device: torch.unique(return_inverse=True, return_counts=True), index_add_, scatter_reduce('amax').  Both
sides alternate inside one process; every figure is a device-event time over `--steps` calls after `--warmup` calls, the
median of `--repeats` windows, in milliseconds per call.  A measurement, not a gate: prints one JSON line.

    python benchmarks/dyn_voxel.py [--scenes 8] [--points 180000] [--steps 20] [--warmup 5] [--repeats 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pdanet_amd import dyn_voxel_utils as dvu                      # noqa: E402
from pdanet_amd.dynamic_vfe import DynamicMeanVFE, DynamicPillarVFE      # noqa: E402

SETTINGS = {
    "voxel": dict(voxel_size=[0.1, 0.1, 0.15], range=[-75.2, -75.2, -2, 75.2, 75.2, 4], pillars=False),
    "pillar": dict(voxel_size=[0.32, 0.32, 6], range=[-74.88, -74.88, -2, 74.88, 74.88, 4], pillars=True),
}
PILLAR_CFG = {"USE_NORM": True, "WITH_DISTANCE": False, "USE_ABSLOTE_XYZ": True, "NUM_FILTERS": [64, 64]}


def make_points(scenes, per_scene, seed=0):
    """A sweep-like cloud: dense near the sensor, thinning with range, some rows outside the range; scenes interleaved."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = scenes * per_scene
    r = 80.0 * torch.rand(n, generator=g, device="cuda") ** 1.7
    a = 6.2831853 * torch.rand(n, generator=g, device="cuda")
    pts = torch.empty((n, 6), device="cuda")
    pts[:, 0] = torch.randint(0, scenes, (n,), generator=g, device="cuda").float()
    pts[:, 1], pts[:, 2] = r * torch.cos(a), r * torch.sin(a)
    pts[:, 3] = -1.8 + 0.04 * r * torch.randn(n, generator=g, device="cuda").abs() + 0.05 * torch.randn(n, generator=g, device="cuda")
    pts[:, 4:] = torch.rand((n, 2), generator=g, device="cuda")
    return pts


# ---- the torch composition -------------------------------------------------------------------------------------------------
class TorchDynamic:
    """The reference's forward with torch_scatter replaced by index_add_ / scatter_reduce."""

    def __init__(self, setting, batch, vfe=None):
        self.lo = torch.tensor(setting["range"][:3], device="cuda")
        self.vs = torch.tensor(setting["voxel_size"], device="cuda")
        spec = dvu.DynVoxelSpec(setting["range"], setting["voxel_size"])
        self.grid = torch.tensor(spec.grid.tolist(), device="cuda")
        self.g = [int(v) for v in spec.grid]
        self.pillars, self.vfe, self.setting = setting["pillars"], vfe, setting

    def index(self, points):
        k = 2 if self.pillars else 3
        coords = torch.floor((points[:, 1:1 + k] - self.lo[:k]) / self.vs[:k]).int()
        mask = ((coords >= 0) & (coords < self.grid[:k])).all(dim=1)
        points, coords = points[mask], coords[mask]
        gx, gy, gz = self.g
        if self.pillars:
            key = points[:, 0].int() * (gx * gy) + coords[:, 0] * gy + coords[:, 1]
        else:
            key = points[:, 0].int() * (gx * gy * gz) + coords[:, 0] * (gy * gz) + coords[:, 1] * gz + coords[:, 2]
        unq, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
        return points, coords, unq, inv, cnt

    def mean(self, src, inv, cnt):
        out = torch.zeros((cnt.shape[0], src.shape[1]), device="cuda")
        out.index_add_(0, inv, src)
        return out / cnt.unsqueeze(1).float()

    def forward_mean(self, points):
        points, _, unq, inv, cnt = self.index(points)
        gx, gy, gz = self.g
        feats = self.mean(points[:, 1:].contiguous(), inv, cnt)
        coords = torch.stack((unq // (gx * gy * gz), (unq % (gx * gy * gz)) // (gy * gz), (unq % (gy * gz)) // gz, unq % gz), 1)
        return feats, coords[:, [0, 3, 2, 1]].contiguous()

    def forward_pillar(self, points):
        points, coords, unq, inv, cnt = self.index(points)
        gx, gy, _ = self.g
        xyz = points[:, 1:4].contiguous()
        f_cluster = xyz - self.mean(xyz, inv, cnt)[inv]
        vs, lo = self.setting["voxel_size"], self.setting["range"]
        f_center = torch.stack((xyz[:, 0] - (coords[:, 0].float() * vs[0] + (vs[0] / 2 + lo[0])),
                                xyz[:, 1] - (coords[:, 1].float() * vs[1] + (vs[1] / 2 + lo[1])),
                                xyz[:, 2] - (vs[2] / 2 + lo[2])), 1)
        x = torch.cat([points[:, 1:], f_cluster, f_center], 1)
        for pfn in self.vfe.pfn_layers:
            x = pfn.relu(pfn.norm(pfn.linear(x)))
            x_max = torch.zeros((cnt.shape[0], x.shape[1]), device="cuda").scatter_reduce(
                0, inv.unsqueeze(1).expand(-1, x.shape[1]), x, "amax", include_self=False)
            x = x_max if pfn.last_vfe else torch.cat([x, x_max[inv]], 1)
        zero = torch.zeros_like(unq)
        coords = torch.stack((unq // (gx * gy), zero, unq % gy, (unq % (gx * gy)) // gy), 1)
        return x, coords


def timed(fn, steps, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        windows.append(t0.elapsed_time(t1) / steps)
    windows.sort()
    return windows[len(windows) // 2], windows[0], windows[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--points", type=int, default=180000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--index-only", action="store_true", help="run the index stage alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/dyn_voxel.py needs the GPU: a CPU run gives no time")
    torch.cuda.set_device(0)
    points = make_points(args.scenes, args.points)
    result = {"benchmark": "dyn_voxel", "scenes": args.scenes, "points_per_scene": args.points, "columns": 5, "steps": args.steps,
              "warmup": args.warmup, "repeats": args.repeats, "unit": "ms per call (median, min, max of the windows)"}
    with torch.no_grad():
        for name, setting in SETTINGS.items():
            spec = dvu.DynVoxelSpec(setting["range"], setting["voxel_size"])
            if args.index_only:
                for _ in range(args.warmup + args.steps):
                    dvu.dynamic_voxel_index(points, spec, args.scenes, setting["pillars"])
                torch.cuda.synchronize()
                continue
            grid = spec.grid.tolist()
            if setting["pillars"]:
                vfe = DynamicPillarVFE(PILLAR_CFG, 5, setting["voxel_size"], grid, setting["range"]).cuda().train()
            else:
                vfe = DynamicMeanVFE({}, 5, setting["voxel_size"], grid, setting["range"])
            ref = TorchDynamic(setting, args.scenes, vfe)
            ref_forward = ref.forward_pillar if setting["pillars"] else ref.forward_mean
            key = "pillar_features" if setting["pillars"] else "voxel_features"
            # the two sides group the same points (the sums differ in order, so features agree to rounding only)
            out = vfe({"points": points, "batch_size": args.scenes})
            feats, coords = ref_forward(points)
            assert torch.equal(out["voxel_coords"].long(), coords.long()), name
            err = float((out[key] - feats).abs().max())
            index = dvu.dynamic_voxel_index(points, spec, args.scenes, setting["pillars"])
            kept, voxels = index.counts.tolist()
            runs = {"index_hip": lambda: dvu.dynamic_voxel_index(points, spec, args.scenes, setting["pillars"]),
                    "index_torch": lambda: ref.index(points),
                    "forward_hip": lambda: vfe({"points": points, "batch_size": args.scenes}),
                    "forward_torch": lambda: ref_forward(points)}
            res = {"kept": kept, "voxels": voxels, "max_abs_feature_difference": err}
            for k, fn in runs.items():
                res[k] = [round(v, 4) for v in timed(fn, args.steps, args.warmup, args.repeats)]
            result[name] = res
    print(json.dumps(result))


if __name__ == "__main__":
    main()
