#!/usr/bin/env python
"""Times the second stage of SECOND-IoU at the sizes kitti_models/second_iou.yaml runs it: the training shape (4 scenes x 128
RoIs) and the eval shape (1 scene x 100 RoIs), C = 512 on a 200 x 176 map, GRID_SIZE 7.

Per shape: the RoI-grid pooling alone, and the head's forward + IoU loss + backward on given RoIs and labels (train mode), each
on the fused path (csrc/bev_roi_pool.hip) and on the composed path, the reference's own affine_grid + grid_sample loop over
the scenes on the same device (PDA_BEV_ROI_POOL=composed).  The composed path is the yardstick.  Also the points-per-box count
of the num_pts_iou_cls score for 100 boxes x 20 000 points (csrc/roi_pool.hip) against the boxes x points mask summed by torch.

The sides alternate inside one process; every figure is a device-event time over `--steps` calls after `--warmup` calls, the
median of `--repeats` windows, in milliseconds per call.  The two pooling paths are compared at the timed sizes before anything
is timed.  A measurement, not a gate: prints one JSON line.

    python benchmarks/second_iou.py [--steps 20] [--warmup 5] [--repeats 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pdanet_amd import second_head                                  # noqa: E402
from pdanet_amd.config import to_attr                               # noqa: E402
from pdanet_amd.roiaware_pool3d_utils import points_in_boxes_count, roiaware_pool3d_cuda      # noqa: E402

PCR, VOXEL = [0, -40, -3, 70.4, 40, 1], [0.05, 0.05, 0.1]
C, H, W = 512, 200, 176
HEAD_CFG = {
    'CLASS_AGNOSTIC': True, 'SHARED_FC': [256, 256], 'IOU_FC': [256, 256], 'DP_RATIO': 0.3,
    'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000, 'NMS_POST_MAXSIZE': 512,
                             'NMS_THRESH': 0.8},
                   'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 1024, 'NMS_POST_MAXSIZE': 100,
                            'NMS_THRESH': 0.7}},
    'ROI_GRID_POOL': {'GRID_SIZE': 7, 'IN_CHANNEL': C, 'DOWNSAMPLE_RATIO': 8},
    'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5, 'SAMPLE_ROI_BY_EACH_CLASS': True,
                      'CLS_SCORE_TYPE': 'roi_iou', 'CLS_FG_THRESH': 0.75, 'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1,
                      'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55},
    'LOSS_CONFIG': {'IOU_LOSS': 'BinaryCrossEntropy', 'LOSS_WEIGHTS': {'rcnn_iou_weight': 1.0, 'code_weights': [1.0] * 7}},
}
SHAPES = {"train_4x128": (4, 128), "eval_1x100": (1, 100)}


def make_rois(scenes, rois, g):
    """Car-, pedestrian- and cyclist-sized boxes over the range, a tenth of them zero rows (the padding of proposal_layer)."""
    dims = torch.tensor([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], device="cuda")
    r = torch.zeros((scenes, rois, 7), device="cuda")
    u = lambda lo, hi: lo + (hi - lo) * torch.rand((scenes, rois), generator=g, device="cuda")
    r[..., 0], r[..., 1], r[..., 2] = u(0, 70.4), u(-40, 40), u(-1.5, -0.5)
    r[..., 3:6] = dims[torch.randint(0, 3, (scenes, rois), generator=g, device="cuda")]
    r[..., 6] = u(-3.14159, 3.14159)
    r[torch.rand((scenes, rois), generator=g, device="cuda") < 0.1] = 0
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
        os.environ[second_head.ENV] = path
        return fn()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/second_iou.py needs the GPU: a CPU run gives no time")
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    result = {"benchmark": "second_iou", "channels": C, "map": [H, W], "grid_size": 7, "steps": args.steps, "warmup": args.warmup,
              "repeats": args.repeats, "unit": "ms per call (median, min, max of the windows)"}
    torch.manual_seed(0)
    head = second_head.SECONDHead(backbone_channels={}, model_cfg=to_attr(HEAD_CFG), point_cloud_range=PCR, voxel_size=VOXEL,
                                  num_class=1).cuda().train()
    for name, (scenes, n_rois) in SHAPES.items():
        bev = torch.randn((scenes, C, H, W), generator=g, device="cuda")
        batch = {'batch_size': scenes, 'rois': make_rois(scenes, n_rois, g), 'spatial_features_2d': bev}
        labels = torch.rand((scenes, n_rois), generator=g, device="cuda")
        pool = lambda: head.roi_grid_pool(batch)

        def step():
            head.zero_grad(set_to_none=True)
            pooled = head.roi_grid_pool(batch)
            rcnn_iou = head.iou_layers(head.shared_fc_layer(pooled.view(pooled.shape[0], -1, 1))).transpose(1, 2).contiguous().squeeze(dim=1)
            loss, _ = head.get_box_iou_layer_loss({'rcnn_iou': rcnn_iou, 'rcnn_cls_labels': labels})
            loss.backward()
            return loss

        a, b = on_path("fused", pool)(), on_path("composed", pool)()
        res = {"rois": [scenes, n_rois], "output_megabytes": round(a.numel() * 4 / 1e6, 2),
               "max_abs_difference_fused_composed": float((a - b).abs().max()), "max_abs_output": float(b.abs().max())}
        del a, b
        res.update(timed_alternating({"pool_fused": on_path("fused", pool), "pool_composed": on_path("composed", pool),
                                      "head_fwd_bwd_fused": on_path("fused", step), "head_fwd_bwd_composed": on_path("composed", step)},
                                     args.steps, args.warmup, args.repeats))
        result[name] = res
    n_pts, n_boxes = 20000, 100
    points = torch.cat([torch.zeros((n_pts, 1), device="cuda"),
                        torch.rand((n_pts, 3), generator=g, device="cuda") * torch.tensor([70.4, 80.0, 4.0], device="cuda")
                        + torch.tensor([0.0, -40.0, -3.0], device="cuda"), torch.rand((n_pts, 1), generator=g, device="cuda")], 1)
    boxes = make_rois(1, n_boxes, g)
    xyz = points[:, 1:4].contiguous()

    def mask_then_sum():
        mask = torch.zeros((n_boxes, n_pts), dtype=torch.int32, device="cuda")
        roiaware_pool3d_cuda.points_in_boxes_cpu(boxes[0], xyz, mask)
        return mask.sum(dim=1)

    count = lambda: points_in_boxes_count(points, boxes)
    assert torch.equal(count()[0].long(), mask_then_sum().long())
    res = {"boxes": n_boxes, "points": n_pts, "points_inside_any_box": int(count().sum())}
    res.update(timed_alternating({"count_hip": count, "mask_then_sum": mask_then_sum}, args.steps, args.warmup, args.repeats))
    result["points_per_box"] = res
    os.environ.pop(second_head.ENV, None)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
