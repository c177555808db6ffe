#!/usr/bin/env python
"""Times the augmentor's ordered step program (pdanet_amd.data_augmentor.DataAugmentor on a list that holds local steps,
csrc/augment_steps.hip) on the scenes of tools/augment_bench.py: 2 ONCE-like scenes of 100 000 raw points and 20 boxes, a
database of 300 objects.  The step list is that of the reference's tools/cfgs/kitti_models/pointpillar_newaugs.yaml, all
ten steps enabled (gt_sampling with the ONCE yaml's groups, local rotation, local scaling, flip, rotation, scaling,
translation on x, y, z, local translation on x, y, z, world dropout top, local dropout top): 13 ops, 10 launches.

  device_steps_ms    the program path from Python: device inputs, check=False, a new plan drawn on the host every call,
                     device events over --iters calls after --warmup calls
  device_legacy_ms   the ONCE yaml's four-step list (the pda_augment path), timed the same way in the same process
  numpy_steps_ms     the same chain in numpy on one core: augment_bench's paste, then the steps box by box, each
                     vectorised over the points -- this tool's own restatement, an estimate of the host cost

Prints one JSON line.  Needs a GPU.  Under `rocprofv3 --kernel-trace --stats` run it with --no-host --iters 100.

    python tools/augment_steps_bench.py [--iters 200] [--warmup 20] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import augment_bench as ab  # noqa: E402
from pdanet_amd import config, data_augmentor  # noqa: E402

f32 = np.float32


def step_list(sampler_cfg):
    return [sampler_cfg,
            {"NAME": "random_local_rotation", "LOCAL_ROT_ANGLE": [-0.15707963267, 0.15707963267]},
            {"NAME": "random_local_scaling", "LOCAL_SCALE_RANGE": [0.95, 1.05]},
            {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x"]},
            {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
            {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [0.95, 1.05]},
            {"NAME": "random_world_translation", "NOISE_TRANSLATE_STD": 0.2, "ALONG_AXIS_LIST": ["x", "y", "z"]},
            {"NAME": "random_local_translation", "LOCAL_TRANSLATION_RANGE": [0.95, 1.05], "ALONG_AXIS_LIST": ["x", "y", "z"]},
            {"NAME": "random_world_frustum_dropout", "INTENSITY_RANGE": [0, 0.2], "DIRECTION": ["top"]},
            {"NAME": "random_local_frustum_dropout", "INTENSITY_RANGE": [0, 0.2], "DIRECTION": ["top"]}]


def _cs(a):
    return f32(np.cos(np.float64(a))), f32(np.sin(np.float64(a)))


def _rot(x, y, c, s):
    return x * c + y * (-s), x * s + y * c


def numpy_steps(P, bx, ops, scene_draws, box_draws):
    """The program on one pasted scene (points (n, C), boxes (m, 8)), in float32 numpy, box by box."""
    pi = f32(np.pi)
    local = 0
    for (code, arg), d in zip(ops.tolist(), scene_draws.tolist()):
        if code == 0:
            if d != 0:
                P[:, 1], bx[:, 1], bx[:, 6] = -P[:, 1], -bx[:, 1], -bx[:, 6]
        elif code == 1:
            if d != 0:
                P[:, 0], bx[:, 0], bx[:, 6] = -P[:, 0], -bx[:, 0], -(bx[:, 6] + pi)
        elif code == 2:
            if f32(d) != 0:
                c, s = _cs(f32(d))
                P[:, 0], P[:, 1] = _rot(P[:, 0].copy(), P[:, 1].copy(), c, s)
                bx[:, 0], bx[:, 1] = _rot(bx[:, 0].copy(), bx[:, 1].copy(), c, s)
                bx[:, 6] = bx[:, 6] + f32(d)
        elif code == 3:
            P[:, :3] *= f32(d)
            bx[:, :6] *= f32(d)
        elif code == 4:
            P[:, arg] += d
            bx[:, arg] += d
        elif code == 5:
            col = 2 if arg < 2 else 1
            mx, mn = P[:, col].max(), P[:, col].min()
            thr = mx - f32(d) * (mx - mn) if arg in (0, 2) else mn + f32(d) * (mx - mn)
            P, bx = (P[P[:, col] < thr], bx[bx[:, col] < thr]) if arg in (0, 2) else (P[P[:, col] > thr], bx[bx[:, col] > thr])
        else:
            row = box_draws[local]
            local += 1
            for j in range(len(bx)):
                f = f32(row[j])
                cx, cy, cz, dx, dy, dz, h = bx[j, :7]
                ca, sa = _cs(-h)
                sx, sy, sz = P[:, 0] - cx, P[:, 1] - cy, P[:, 2] - cz
                lx, ly = _rot(sx, sy, ca, sa)
                m = (np.abs(sz) <= dz / 2) & (np.abs(lx) <= dx / 2 + f32(0.1)) & (np.abs(ly) <= dy / 2 + f32(0.1))
                if code == 6:
                    P[m, arg] += f
                    bx[j, arg] += f
                elif code == 7:
                    x, y = _rot(sx[m], sy[m], *_cs(f))
                    P[m, 0], P[m, 1], P[m, 2] = x + cx, y + cy, sz[m] + cz
                    bx[j, 6] = h + f
                elif code == 8:
                    P[m, 0], P[m, 1], P[m, 2] = sx[m] * f + cx, sy[m] * f + cy, sz[m] * f + cz
                    bx[j, 3:6] *= f
                else:
                    ctr, ext, col = (cz, dz, 2) if arg < 2 else (cy, dy, 1)
                    hit = P[:, col] >= (ctr + ext / 2) - f * ext if arg in (0, 2) else P[:, col] <= (ctr - ext / 2) + f * ext
                    P = P[~(m & hit)]
    bx[:, 6] = bx[:, 6] - np.floor(bx[:, 6] / f32(2 * np.pi) + f32(0.5)) * f32(2 * np.pi)
    return P, bx[bx[:, 7] != 0]


def numpy_chain(aug, paste_aug, db_boxes, db_points, db_cls, pts, boxes, cls, plan):
    """augment_bench's numpy paste with the identity transform, class-0 boxes kept, then the steps."""
    B = len(pts)
    ident = dict(plan, flip_x=np.zeros(B, np.int32), flip_y=np.zeros(B, np.int32), angle=np.zeros(B), scale=np.ones(B, f32))
    keep_all = [np.ones(len(c), np.int32) for c in cls]
    pasted = ab.numpy_augment(paste_aug, db_boxes, db_points, pts, boxes, keep_all, ident)
    ops, scene_draws, box_draws, _ = aug._program_draws(plan, B, np.asarray(plan["flip_x"]), np.asarray(plan["flip_y"]),
                                                         np.asarray(plan["angle"], np.float64), np.asarray(plan["scale"], f32))
    out = []
    for b, (p, bx) in enumerate(pasted):
        n_acc = len(bx) - len(boxes[b])
        col = np.concatenate([cls[b].astype(f32), np.ones(n_acc, f32)])     # the class of a pasted box does not matter here
        out.append(numpy_steps(p, np.concatenate([bx, col.reshape(-1, 1)], 1), ops, scene_draws[b], box_draws[b]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "augment_steps_bench needs a GPU"
    cfg = config.load_yaml("once_pda_ssd.yaml")
    rng = np.random.default_rng(0)
    dbb, dbp = ab.database(rng)
    db = data_augmentor.GtDatabase.from_arrays(ab.NAMES, dbb, dbp)
    legacy = data_augmentor.from_config(cfg, db)
    aug_cfg = cfg["DATA_CONFIG"]["DATA_AUGMENTOR"]
    sampler_cfg = [c for c in aug_cfg["AUG_CONFIG_LIST"] if c["NAME"] == "gt_sampling"][0]
    aug = data_augmentor.DataAugmentor(step_list(sampler_cfg), ab.NAMES, db)
    pts, boxes, cls = ab.scenes(rng)
    n_cap = max(len(p) for p in pts)
    packed = torch.from_numpy(np.concatenate(pts)).cuda()
    offs = torch.tensor([0, len(pts[0]), len(pts[0]) + len(pts[1])], dtype=torch.int64, device="cuda")
    bx = torch.from_numpy(np.concatenate(boxes)).cuda()
    boffs = torch.tensor([0, len(boxes[0]), len(boxes[0]) + len(boxes[1])], dtype=torch.int64, device="cuda")
    torch.manual_seed(0)

    def timed(which):
        for i in range(a.warmup):
            which((packed, offs, n_cap), (bx, boffs), cls, check=False)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.iters):
            which((packed, offs, n_cap), (bx, boffs), cls, check=False)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    steps_ms = timed(aug)
    legacy_ms = timed(legacy)
    info = aug((packed, offs, n_cap), (bx, boffs), cls, check=False)[2].cpu().numpy()
    res = {"scenes": 2, "raw_points": [len(p) for p in pts], "db_objects": db.n_obj, "ops": len(aug.program),
           "launches": 4 + 4 + 2 * sum(1 for st in aug.program if st[0] == data_augmentor.OP_WDROP),
           "accepted_last": info[:, 2].tolist(), "points_out_last": info[:, 0].tolist(), "boxes_out_last": info[:, 1].tolist(),
           "status_last": info[:, 3].tolist(), "device_steps_ms": round(steps_ms, 4), "device_legacy_ms": round(legacy_ms, 4)}
    if not a.no_host:
        db_boxes = np.concatenate([dbb[n] for n in ab.NAMES])
        db_points = [p for n in ab.NAMES for p in dbp[n]]
        plans = [aug.make_plan(cls, np.random.default_rng(i)) for i in range(a.host_iters + 1)]
        numpy_chain(aug, legacy, db_boxes, db_points, None, pts, boxes, cls, plans[0])
        t0 = time.perf_counter()
        for i in range(a.host_iters):
            out = numpy_chain(aug, legacy, db_boxes, db_points, None, pts, boxes, cls, plans[i + 1])
        res["numpy_steps_ms"] = round((time.perf_counter() - t0) * 1e3 / a.host_iters, 3)
        res["numpy_points_out_last"] = [len(o[0]) for o in out]
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
