#!/usr/bin/env python
"""Times the second stage of PointRCNN at the sizes kitti_models/pointrcnn.yaml runs it: the training shape (2 scenes x 128
RoIs) and the eval shape (1 scene x 100 RoIs), N = 16 384 points a scene, C = 128, 512 sampled points a RoI.

Per shape: the head's input stage alone (roipool3d_gpu), and the head's forward + losses + backward on given RoIs and targets
(train mode), each on the fused path (csrc/roi_pool.hip, roipoint_pool_canonical_kernel) and on the composed path, the
reference's own norm + cat + enlarge + fills + pooling + subtraction + rotation + masked zero on the same device
(PDA_ROIPOINT_POOL=composed).  The composed path is the yardstick.  Also the detector's training iteration (forward, losses,
backward) at 2 x 16 384 points on both paths.

The sides alternate inside one process; every figure is a device-event time over `--steps` calls after `--warmup` calls, the
median of `--repeats` windows, in milliseconds per call.  The two pooling paths are compared at the timed sizes before anything
is timed.  A measurement, not a gate: prints one JSON line.

    python benchmarks/pointrcnn.py [--steps 10] [--warmup 3] [--repeats 5] [--no-detector]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.second_iou import timed_alternating                # noqa: E402
from pdanet_amd import pointrcnn_head                               # noqa: E402
from pdanet_amd.config import to_attr                               # noqa: E402
from pdanet_amd.point_rcnn import PointRCNN                         # noqa: E402

N_POINTS, C = 16384, 128
MEAN_SIZE = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]
MODEL_CFG = {
    'NAME': 'PointRCNN',
    'BACKBONE_3D': {'NAME': 'PointNet2MSG',
                    'SA_CONFIG': {'NPOINTS': [4096, 1024, 256, 64], 'RADIUS': [[0.1, 0.5], [0.5, 1.0], [1.0, 2.0], [2.0, 4.0]],
                                  'NSAMPLE': [[16, 32], [16, 32], [16, 32], [16, 32]],
                                  'MLPS': [[[16, 16, 32], [32, 32, 64]], [[64, 64, 128], [64, 96, 128]],
                                           [[128, 196, 256], [128, 196, 256]], [[256, 256, 512], [256, 384, 512]]]},
                    'FP_MLPS': [[128, 128], [256, 256], [512, 512], [512, 512]]},
    'POINT_HEAD': {'NAME': 'PointHeadBox', 'CLS_FC': [256, 256], 'REG_FC': [256, 256], 'CLASS_AGNOSTIC': False,
                   'USE_POINT_FEATURES_BEFORE_FUSION': False,
                   'TARGET_CONFIG': {'GT_EXTRA_WIDTH': [0.2, 0.2, 0.2], 'BOX_CODER': 'PointResidualCoder',
                                     'BOX_CODER_CONFIG': {'use_mean_size': True, 'mean_size': MEAN_SIZE}},
                   'LOSS_CONFIG': {'LOSS_REG': 'WeightedSmoothL1Loss',
                                   'LOSS_WEIGHTS': {'point_cls_weight': 1.0, 'point_box_weight': 1.0, 'code_weights': [1.0] * 8}}},
    'ROI_HEAD': {'NAME': 'PointRCNNHead', 'CLASS_AGNOSTIC': True,
                 'ROI_POINT_POOL': {'POOL_EXTRA_WIDTH': [0.0, 0.0, 0.0], 'NUM_SAMPLED_POINTS': 512, 'DEPTH_NORMALIZER': 70.0},
                 'XYZ_UP_LAYER': [128, 128], 'CLS_FC': [256, 256], 'REG_FC': [256, 256], 'DP_RATIO': 0.0, 'USE_BN': False,
                 'SA_CONFIG': {'NPOINTS': [128, 32, -1], 'RADIUS': [0.2, 0.4, 100], 'NSAMPLE': [16, 16, 16],
                               'MLPS': [[128, 128, 128], [128, 128, 256], [256, 256, 512]]},
                 'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                                          'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
                                'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                                         'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.85}},
                 'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5, 'SAMPLE_ROI_BY_EACH_CLASS': True,
                                   'CLS_SCORE_TYPE': 'cls', 'CLS_FG_THRESH': 0.6, 'CLS_BG_THRESH': 0.45, 'CLS_BG_THRESH_LO': 0.1,
                                   'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55},
                 'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                                 'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,
                                                  'code_weights': [1.0] * 7}}},
    'POST_PROCESSING': {'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'SCORE_THRESH': 0.1, 'OUTPUT_RAW_SCORE': False, 'EVAL_METRIC': 'kitti',
                        'NMS_CONFIG': {'MULTI_CLASSES_NMS': False, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.1, 'NMS_PRE_MAXSIZE': 4096,
                                       'NMS_POST_MAXSIZE': 500}},
}
DATASET = {'class_names': ['Car', 'Pedestrian', 'Cyclist'], 'num_point_features': 4}
SHAPES = {"train_2x128": (2, 128), "eval_1x100": (1, 100)}


def make_scene(scenes, g):
    """points over the KITTI range, a third of them in clusters of object size, and the clusters' boxes"""
    u = lambda n, lo, hi: lo + (hi - lo) * torch.rand((scenes, n), generator=g, device="cuda")
    n_obj = 24
    dims = torch.tensor(MEAN_SIZE, device="cuda")
    cls = torch.randint(0, 3, (scenes, n_obj), generator=g, device="cuda")
    boxes = torch.cat([torch.stack([u(n_obj, 5, 65), u(n_obj, -35, 35), u(n_obj, -1.5, -0.5)], dim=-1), dims[cls],
                       u(n_obj, -3.14159, 3.14159).unsqueeze(-1), (cls + 1).float().unsqueeze(-1)], dim=-1)      # (scenes, n_obj, 8)
    n_cl = N_POINTS // 3
    owner = torch.randint(0, n_obj, (scenes, n_cl), generator=g, device="cuda")
    own = torch.gather(boxes, 1, owner.unsqueeze(-1).expand(-1, -1, 8))
    near = own[..., 0:3] + (torch.rand((scenes, n_cl, 3), generator=g, device="cuda") - 0.5) * own[..., 3:6]
    far = torch.stack([u(N_POINTS - n_cl, 0, 70.4), u(N_POINTS - n_cl, -40, 40), u(N_POINTS - n_cl, -3, 1)], dim=-1)
    xyz = torch.cat([near, far], dim=1)
    xyz = xyz[:, torch.randperm(N_POINTS, generator=g, device="cuda")]
    return xyz.contiguous(), boxes


def make_rois(boxes, n_rois, g):
    """the scene's boxes jittered, a tenth of the rows zero (the padding of proposal_layer)"""
    scenes, n_obj = boxes.shape[:2]
    pick = torch.randint(0, n_obj, (scenes, n_rois), generator=g, device="cuda")
    rois = torch.gather(boxes[..., :7], 1, pick.unsqueeze(-1).expand(-1, -1, 7)).clone()
    rois[..., 0:3] += (torch.rand((scenes, n_rois, 3), generator=g, device="cuda") - 0.5) * 0.6
    rois[..., 6] += (torch.rand((scenes, n_rois), generator=g, device="cuda") - 0.5) * 0.3
    rois[torch.rand((scenes, n_rois), generator=g, device="cuda") < 0.1] = 0
    return rois


def on_path(path, fn):
    def run():
        os.environ[pointrcnn_head.ENV] = path
        return fn()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-detector", action="store_true", help="skip the detector's training iteration")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/pointrcnn.py needs the GPU: a CPU run gives no time")
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    result = {"benchmark": "pointrcnn", "points": N_POINTS, "channels": C, "sampled_points": 512, "steps": args.steps,
              "warmup": args.warmup, "repeats": args.repeats, "unit": "ms per call (median, min, max of the windows)"}
    torch.manual_seed(0)
    model = PointRCNN(to_attr(MODEL_CFG), 3, DATASET).cuda().train()
    head = model.roi_head
    for name, (scenes, n_rois) in SHAPES.items():
        xyz, boxes = make_scene(scenes, g)
        rois = make_rois(boxes, n_rois, g)
        coords = torch.cat([torch.arange(scenes, device="cuda").repeat_interleave(N_POINTS).float().unsqueeze(-1), xyz.view(-1, 3)], dim=1)
        batch = {'batch_size': scenes, 'rois': rois, 'roi_scores': torch.zeros((scenes, n_rois), device="cuda"),
                 'roi_labels': torch.ones((scenes, n_rois), dtype=torch.long, device="cuda"), 'gt_boxes': boxes,
                 'point_coords': coords, 'point_features': torch.randn((scenes * N_POINTS, C), generator=g, device="cuda"),
                 'point_cls_scores': torch.rand((scenes * N_POINTS,), generator=g, device="cuda")}
        pool = lambda: head.roipool3d_gpu(batch)

        def step():
            head.zero_grad(set_to_none=True)
            head(dict(batch, roi_target_seed=3))
            loss, _ = head.get_loss()
            loss.backward()
            return loss

        a, b = on_path("fused", pool)(), on_path("composed", pool)()
        res = {"rois": [scenes, n_rois], "output_megabytes": round(a.numel() * 4 / 1e6, 2),
               "empty_rois": int((a.abs().amax(dim=(1, 2)) == 0).sum()),
               "max_abs_difference_fused_composed": float((a - b).abs().max()), "max_abs_output": float(b.abs().max())}
        del a, b
        fns = {"pool_fused": on_path("fused", pool), "pool_composed": on_path("composed", pool)}
        if n_rois >= MODEL_CFG['ROI_HEAD']['TARGET_CONFIG']['ROI_PER_IMAGE']:      # the training shape: targets are sampled from the RoIs
            fns.update({"head_fwd_bwd_fused": on_path("fused", step), "head_fwd_bwd_composed": on_path("composed", step)})
        res.update(timed_alternating(fns, args.steps, args.warmup, args.repeats))
        result[name] = res
    if not args.no_detector:
        scenes = 2
        xyz, boxes = make_scene(scenes, g)
        points = torch.cat([torch.arange(scenes, device="cuda").repeat_interleave(N_POINTS).float().unsqueeze(-1), xyz.view(-1, 3),
                            torch.rand((scenes * N_POINTS, 1), generator=g, device="cuda")], dim=1)
        batch = {'batch_size': scenes, 'points': points, 'gt_boxes': boxes}

        def iteration():
            model.zero_grad(set_to_none=True)
            ret, _, _ = model(dict(batch, roi_target_seed=3))
            ret['loss'].backward()
            return ret['loss']

        res = {"scenes": scenes, "parameters": sum(p.numel() for p in model.parameters())}
        res.update(timed_alternating({"train_iteration_fused": on_path("fused", iteration),
                                      "train_iteration_composed": on_path("composed", iteration)}, args.steps, args.warmup, args.repeats))
        result["detector_2x16384"] = res
    os.environ.pop(pointrcnn_head.ENV, None)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
