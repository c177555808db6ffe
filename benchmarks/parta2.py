#!/usr/bin/env python
"""Times Part-A2 at the training shape of kitti_models/PartA2.yaml: 4 scenes of about 16 000 voxels on the 1408 x 1600 x 40 grid,
4 x 128 RoIs, POOL_SIZE 12, MAX_POINTS_PER_VOXEL 128, 16 point-feature channels.

  input stage   PartA2FCHead's roiaware_pool (collection, both poolings, the sparse rows of the live voxels), forward alone and
                forward + backward, on the fused path (csrc/parta2.hip pda_parta2_pool_*) and on the composed path
                (PDA_PARTA2_POOL=composed: per-scene masks, two RoIAwarePool3d calls, nonzero, indexing).  The composed path is
                the yardstick; the two are compared bit for bit in the forward before anything is timed.
  UNetV2        forward and forward + backward (sum of squares of point_features and the encoded tensor).
  PartA2Net     one training iteration (forward, loss, backward) of the yaml's model on the fused path and on the composed one.

The model settings are the yaml's MODEL block as tests/golden/parta2_state_dict.json records it.  The sides alternate inside one
process; every figure is a device-event time over `--steps` calls after `--warmup` calls, the median of `--repeats` windows, in
milliseconds per call.  A measurement, not a gate: prints one JSON line.

    python benchmarks/parta2.py [--steps 10] [--warmup 3] [--repeats 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pdanet_amd.config import to_attr                               # noqa: E402
from pdanet_amd.part_a2_net import PartA2Net                        # noqa: E402
from pdanet_amd.parta2_head import PartA2FCHead                     # noqa: E402
from pdanet_amd.spconv_unet import UNetV2                           # noqa: E402
from pdanet_amd.voxel_utils import get_voxel_centers                # noqa: E402

ENV = 'PDA_PARTA2_POOL'
PCR, VOXEL, GRID = [0, -40, -3, 70.4, 40, 1], [0.05, 0.05, 0.1], [1408, 1600, 40]
DATASET = {'class_names': ['Car', 'Pedestrian', 'Cyclist'], 'point_cloud_range': PCR, 'voxel_size': VOXEL, 'num_point_features': 4}
SCENES, ROIS, VOXELS_PER_SCENE, OBJECTS = 4, 128, 16000, 12


def model_settings():
    with open(os.path.join(ROOT, "tests", "golden", "parta2_state_dict.json")) as f:
        return json.load(f)['config']['MODEL']


def make_scene_voxels(g):
    """(coords (N, 4) int32 [b, z, y, x] scene-major without duplicates, object centres (SCENES, OBJECTS, 3)): per scene a ground
    sheet and OBJECTS car-sized clusters, about VOXELS_PER_SCENE distinct voxels."""
    rows, centres = [], []
    for b in range(SCENES):
        u = lambda n, lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, device="cuda")
        c = torch.stack([u(OBJECTS, 5, 65), u(OBJECTS, -35, 35), u(OBJECTS, -1.2, -0.8)], 1)
        n_obj = VOXELS_PER_SCENE // 2 // OBJECTS
        obj = c.repeat_interleave(n_obj, 0) + (torch.rand((OBJECTS * n_obj, 3), generator=g, device="cuda") - 0.5) * \
            torch.tensor([3.9, 1.6, 1.5], device="cuda")
        n_ground = VOXELS_PER_SCENE * 6 // 10
        ground = torch.stack([u(n_ground, 0, 70.4), u(n_ground, -40, 40), u(n_ground, -1.8, -1.6)], 1)
        xyz = torch.cat([obj, ground])
        idx = ((xyz - torch.tensor(PCR[:3], device="cuda")) / torch.tensor(VOXEL, device="cuda")).floor().long()
        idx = idx.clamp(min=torch.zeros(3, dtype=torch.long, device="cuda"), max=torch.tensor(GRID, device="cuda") - 1)
        key = torch.unique((idx[:, 2] * GRID[1] + idx[:, 1]) * GRID[0] + idx[:, 0])
        rows.append(torch.stack([torch.full_like(key, b), key // (GRID[1] * GRID[0]), (key // GRID[0]) % GRID[1], key % GRID[0]], 1))
        centres.append(c)
    return torch.cat(rows).int().contiguous(), torch.stack(centres)


def make_rois(centres, g):
    """(SCENES, ROIS, 7): car-sized boxes scattered around the object centres, a tenth of them zero rows (proposal_layer's padding)."""
    pick = torch.randint(0, OBJECTS, (SCENES, ROIS), generator=g, device="cuda")
    r = torch.zeros((SCENES, ROIS, 7), device="cuda")
    r[..., 0:3] = torch.gather(centres, 1, pick.unsqueeze(-1).expand(-1, -1, 3)) + \
        (torch.rand((SCENES, ROIS, 3), generator=g, device="cuda") - 0.5) * torch.tensor([1.0, 0.6, 0.3], device="cuda")
    r[..., 3:6] = torch.tensor([3.9, 1.6, 1.56], device="cuda") * (0.9 + 0.2 * torch.rand((SCENES, ROIS, 3), generator=g, device="cuda"))
    r[..., 6] = (torch.rand((SCENES, ROIS), generator=g, device="cuda") - 0.5) * 6.28318
    r[torch.rand((SCENES, ROIS), generator=g, device="cuda") < 0.1] = 0
    return r


def timed_alternating(fns, steps, warmup, repeats):
    """name -> [median, min, max] ms per call; the sides take turns, one window each, `repeats` times."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    windows = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            windows[k].append(t0.elapsed_time(t1) / steps)
    out = {}
    for k, w in windows.items():
        w.sort()
        out[k] = [round(w[len(w) // 2], 4), round(w[0], 4), round(w[-1], 4)]
    return out


def on_path(path, fn):
    def run():
        os.environ[ENV] = path
        return fn()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-net", action="store_true", help="leave the PartA2Net training iteration out")
    args = ap.parse_args()
    settings = model_settings()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/parta2.py needs the GPU: a CPU run gives no time")
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    torch.manual_seed(0)
    result = {"benchmark": "parta2", "scenes": SCENES, "rois_per_scene": ROIS, "steps": args.steps, "warmup": args.warmup,
              "repeats": args.repeats, "unit": "ms per call (median, min, max of the windows)"}
    coords, centres = make_scene_voxels(g)
    n = coords.shape[0]
    result["voxels"] = [int((coords[:, 0] == b).sum()) for b in range(SCENES)]

    # ---- the head's input stage ------------------------------------------------------------------------------------------------
    head = PartA2FCHead(input_channels=16, model_cfg=to_attr(settings['ROI_HEAD']), num_class=1).cuda().train()
    pool_cfg = settings['ROI_HEAD']['ROI_AWARE_POOL']
    point_coords = torch.cat((coords[:, 0:1].float(), get_voxel_centers(coords[:, 1:], 1, VOXEL, PCR)), 1).contiguous()
    feats = torch.randn((n, 16), generator=g, device="cuda").requires_grad_(True)
    offset = torch.rand((n, 3), generator=g, device="cuda").requires_grad_(True)
    batch = {'batch_size': SCENES, 'rois': make_rois(centres, g), 'point_coords': point_coords, 'point_features': feats,
             'point_part_offset': offset, 'point_cls_scores': torch.rand(n, generator=g, device="cuda")}
    pool = lambda: head.roiaware_pool(batch)

    def pool_fwd_bwd():
        feats.grad = offset.grad = None
        _, part, rpn = head.roiaware_pool(batch)
        ((part ** 2).sum() + (rpn ** 2).sum()).backward()

    a, b = on_path("fused", pool)(), on_path("composed", pool)()
    res = {"pool_size": pool_cfg['POOL_SIZE'], "max_points_per_voxel": pool_cfg['MAX_POINTS_PER_VOXEL'], "live_voxels": int(a[0].shape[0]),
           "of_voxels": SCENES * ROIS * pool_cfg['POOL_SIZE'] ** 3,
           "forward_bitwise_equal": bool(all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b)))}
    del a, b
    res.update(timed_alternating({"fwd_fused": on_path("fused", pool), "fwd_composed": on_path("composed", pool),
                                  "fwd_bwd_fused": on_path("fused", pool_fwd_bwd), "fwd_bwd_composed": on_path("composed", pool_fwd_bwd)},
                                 args.steps, args.warmup, args.repeats))
    result["input_stage"] = res
    del head, batch, feats, offset
    torch.cuda.empty_cache()

    # ---- UNetV2 ------------------------------------------------------------------------------------------------------------------
    unet = UNetV2(to_attr(settings['BACKBONE_3D']), 4, GRID, VOXEL, PCR).cuda().train()
    vox_feats = torch.randn((n, 4), generator=g, device="cuda")
    inputs = lambda: {'voxel_features': vox_feats, 'voxel_coords': coords, 'batch_size': SCENES}

    def unet_fwd():
        with torch.no_grad():
            return unet(inputs())

    def unet_fwd_bwd():
        unet.zero_grad(set_to_none=True)
        out = unet(inputs())
        ((out['point_features'] ** 2).sum() + (out['encoded_spconv_tensor'].features ** 2).sum()).backward()

    result["unet_v2"] = timed_alternating({"fwd": unet_fwd, "fwd_bwd": unet_fwd_bwd}, args.steps, args.warmup, args.repeats)
    del unet
    torch.cuda.empty_cache()

    # ---- one training iteration of the detector ------------------------------------------------------------------------------------
    if not args.skip_net:
        model = PartA2Net(to_attr(settings), 3, DATASET).cuda().train()
        centre_xyz = point_coords[:, 1:4]
        voxels = centre_xyz.unsqueeze(1) + (torch.rand((n, 5, 3), generator=g, device="cuda") - 0.5) * torch.tensor(VOXEL, device="cuda")
        voxels = torch.cat((voxels, torch.rand((n, 5, 1), generator=g, device="cuda")), -1)
        num_points = torch.randint(1, 6, (n,), generator=g, device="cuda", dtype=torch.int32)
        voxels = voxels * (torch.arange(5, device="cuda").view(1, 5, 1) < num_points.view(-1, 1, 1))
        gt = torch.zeros((SCENES, OBJECTS, 8), device="cuda")
        gt[..., 0:3], gt[..., 7] = centres, 1
        gt[..., 3:6] = torch.tensor([3.9, 1.6, 1.56], device="cuda")
        gt[..., 6] = (torch.rand((SCENES, OBJECTS), generator=g, device="cuda") - 0.5) * 6.28318
        net_batch = {'voxels': voxels.contiguous(), 'voxel_coords': coords, 'voxel_num_points': num_points, 'gt_boxes': gt,
                     'batch_size': SCENES}

        def iteration():
            model.zero_grad(set_to_none=True)
            ret, _, _ = model(dict(net_batch))
            ret['loss'].backward()
            return ret['loss'].detach()

        try:
            loss = float(on_path("fused", iteration)())
            res = {"first_loss": loss, "parameters": sum(p.numel() for p in model.parameters())}
            res.update(timed_alternating({"iteration_fused": on_path("fused", iteration),
                                          "iteration_composed": on_path("composed", iteration)}, args.steps, args.warmup, args.repeats))
        except Exception as exc:                                     # the figures above are still reported
            res = {"error": "%s: %s" % (type(exc).__name__, exc)}
        result["part_a2_net"] = res
    os.environ.pop(ENV, None)
    result["peak_memory_megabytes"] = round(torch.cuda.max_memory_allocated() / 1e6, 1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
