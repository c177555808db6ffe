#!/usr/bin/env python
"""Times CaDDN's FrustumToVoxel at the shape kitti_models/CaDDN.yaml runs it, one image: C = 64 features and D = 80 depth
bins on a 94 x 311 feature map (a 375 x 1242 image at layer1's stride 4), into the 280 x 376 x 25 grid of 0.16 m voxels.

Forward alone and forward + backward (gradients of the image features and the depth logits), each on the fused path
(csrc/frustum_sample.hip) and on the composed path, the reference's frustum tensor + sampling grid + 5-D grid_sample on the same
device (PDA_FRUSTUM_SAMPLE=composed).  The composed path is the yardstick.  Also the peak device memory of one forward +
backward on each path, measured from before the inputs are made, and the forward's floor: the store of the voxel tensor.

The sides alternate inside one process; every time is a device-event time over `--steps` calls after `--warmup` calls, the
median of `--repeats` windows, in milliseconds per call.  The two paths are compared before anything is timed.  A measurement,
not a gate: prints one JSON line.

    python benchmarks/caddn.py [--steps 10] [--warmup 3] [--repeats 5]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.second_iou import timed_alternating                 # noqa: E402
from pdanet_amd import image_vfe                                    # noqa: E402
from pdanet_amd.config import to_attr                               # noqa: E402

PCR, GRID = [2, -30.08, -3.0, 46.8, 30.08, 1.0], [280, 376, 25]
DISC = {"mode": "LID", "num_bins": 80, "depth_min": 2.0, "depth_max": 46.8}
C, HF, WF, IMAGE = 64, 94, 311, (375, 1242)


def calibration():
    """KITTI-like: the camera looks along the LiDAR's x, pitched and yawed by a hundredth of a radian; P2's focal length."""
    a, b = 0.01, -0.01
    rot = torch.tensor([[math.sin(b), -math.cos(b), 0.0, 0.0], [math.sin(a), 0.0, -math.cos(a), -0.08], [math.cos(b), math.sin(b), a, -0.27],
                        [0.0, 0.0, 0.0, 1.0]])
    proj = torch.tensor([[721.5, 0.0, 609.6, 44.9], [0.0, 721.5, 172.9, 0.2], [0.0, 0.0, 1.0, 0.003]])
    return rot[None].cuda().contiguous(), proj[None].cuda().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/caddn.py needs the GPU: a CPU run gives no time")
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    f2v = image_vfe.FrustumToVoxel(to_attr({"SAMPLER": {"mode": "bilinear", "padding_mode": "zeros"}}), GRID, PCR, DISC)
    l2c, c2i = calibration()
    shape = torch.tensor([IMAGE], dtype=torch.int32, device="cuda")

    def make_inputs():
        return (torch.randn((1, C, HF, WF), generator=g, device="cuda").requires_grad_(),
                torch.randn((1, DISC["num_bins"] + 1, HF, WF), generator=g, device="cuda").requires_grad_())

    def forward(feat, logits):
        return f2v({"image_features": feat, "depth_logits": logits, "trans_lidar_to_cam": l2c, "trans_cam_to_img": c2i,
                    "image_shape": shape})["voxel_features"]

    def on_path(path, fn):
        def run():
            os.environ[image_vfe.ENV] = path
            return fn()
        return run

    feat, logits = make_inputs()
    grad_out = torch.randn((1, C, GRID[2], GRID[1], GRID[0]), generator=g, device="cuda")

    def fwd():
        with torch.no_grad():
            return forward(feat, logits)

    def fwd_bwd():
        feat.grad = logits.grad = None
        forward(feat, logits).backward(grad_out)

    a, b = on_path("fused", fwd)(), on_path("composed", fwd)()
    voxel_bytes = a.numel() * 4
    result = {"benchmark": "caddn_frustum_to_voxel", "channels": C, "bins": DISC["num_bins"], "feature_map": [HF, WF], "grid": GRID,
              "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
              "unit": "ms per call (median, min, max of the windows)", "voxel_tensor_megabytes": round(voxel_bytes / 1e6, 1),
              "frustum_tensor_megabytes": round(C * DISC["num_bins"] * HF * WF * 4 / 1e6, 1),
              "share_of_nonzero_voxels": round(float((b != 0).float().mean()), 3),
              "max_abs_difference_fused_composed": float((a - b).abs().max()), "max_abs_output": float(b.abs().max())}
    del a, b
    result.update(timed_alternating({"forward_fused": on_path("fused", fwd), "forward_composed": on_path("composed", fwd),
                                     "fwd_bwd_fused": on_path("fused", fwd_bwd), "fwd_bwd_composed": on_path("composed", fwd_bwd)},
                                    args.steps, args.warmup, args.repeats))
    del feat, logits
    for path in ("fused", "composed"):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        feat, logits = make_inputs()
        os.environ[image_vfe.ENV] = path
        forward(feat, logits).backward(grad_out)
        torch.cuda.synchronize()
        result["peak_megabytes_fwd_bwd_" + path] = round((torch.cuda.max_memory_allocated() - before) / 1e6, 1)
        del feat, logits
    os.environ.pop(image_vfe.ENV, None)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
