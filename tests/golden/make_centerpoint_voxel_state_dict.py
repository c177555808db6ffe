#!/usr/bin/env python
"""Generates tests/golden/centerpoint_voxel_state_dict.json: the state-dict keys and shapes, in order, of the REFERENCE's
voxel CenterPoint -- VoxelResBackBone8x + BaseBEVBackbone + CenterHead under the names Detector3DTemplate.build_networks
registers them with (vfe -- MeanVFE, no parameters --, backbone_3d, map_to_bev_module -- HeightCompression, no parameters --,
backbone_2d, dense_head) -- instantiated on the CPU, plus the settings they were built with.  Names and shapes only.

The reference's own spconv_backbone.py, base_bev_backbone.py and center_head.py (with centernet_utils.py, loss_utils.py and
model_nms_utils.py) are loaded as pcdet_ref.* through reference_loader.py, over the spconv stand-in of
make_second_state_dict.py (modules that hold parameters of spconv 2.x's shapes and compute nothing) and a numba stub.

Two settings, each on a grid of 32 x 32 x 40 cells of its yaml's voxel size:
  kitti     kitti_models/centerpoint.yaml's MODEL block as it is: one head of three classes, FEATURE_MAP_STRIDE 4 (an 8 x 8 map).
  nuscenes  nuscenes_models/cbgs_voxel0075_res3d_centerpoint.yaml's MODEL block -- six heads over ten classes, `vel` in
            HEAD_ORDER, ten code weights, FEATURE_MAP_STRIDE 8 (a 4 x 4 map) -- with the 2D backbone cut to LAYER_NUMS [1, 1];
            points of five features.

Run with the reference checkout:  python tests/golden/make_centerpoint_voxel_state_dict.py /path/to/reference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from reference_loader import (MODEL_UTILS, cpu_torch, extension_stubs, load, model_yaml, reference_root, shapes,  # noqa: E402
                              stub_numba, write_state_dict)
from make_second_state_dict import _spconv_stand_in  # noqa: E402
from pdanet_amd.config import to_attr  # noqa: E402

SETTINGS = {
    "kitti": ("kitti_models/centerpoint.yaml", None,
              {"class_names": ["Car", "Pedestrian", "Cyclist"], "point_cloud_range": [0, -0.8, -3, 1.6, 0.8, 1],
               "voxel_size": [0.05, 0.05, 0.1], "num_point_features": 4}),
    "nuscenes": ("nuscenes_models/cbgs_voxel0075_res3d_centerpoint.yaml", [1, 1],
                 {"class_names": ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle",
                                  "pedestrian", "traffic_cone"],
                  "point_cloud_range": [-1.2, -1.2, -5.0, 1.2, 1.2, 3.0], "voxel_size": [0.075, 0.075, 0.2],
                  "num_point_features": 5}),
}
GRID = [32, 32, 40]


def load_reference(root):
    _spconv_stand_in()
    cpu_torch()
    stub_numba()
    load(root, "pcdet_ref", MODEL_UTILS + ["utils.spconv_utils"], stubs=extension_stubs())
    return load(root, "pcdet_ref", ["models.model_utils.model_nms_utils", "models.model_utils.centernet_utils",
                                    "models.backbones_3d.spconv_backbone", "models.backbones_2d.base_bev_backbone",
                                    "models.dense_heads.center_head"])[2:]


def main():
    root = reference_root()
    b3d, b2d, head = load_reference(root)
    out = {}
    for name, (yaml_name, layer_nums, dataset) in SETTINGS.items():
        model_cfg = model_yaml(root, yaml_name)["MODEL"]
        if layer_nums is not None:
            model_cfg["BACKBONE_2D"]["LAYER_NUMS"] = layer_nums
        cfg = to_attr(model_cfg)
        backbone_3d = getattr(b3d, cfg.BACKBONE_3D.NAME)(cfg.BACKBONE_3D, dataset["num_point_features"], np.array(GRID))
        bev = b2d.BaseBEVBackbone(cfg.BACKBONE_2D, input_channels=cfg.MAP_TO_BEV.NUM_BEV_FEATURES)
        dense_head = head.CenterHead(model_cfg=cfg.DENSE_HEAD, input_channels=bev.num_bev_features,
                                     num_class=len(dataset["class_names"]), class_names=dataset["class_names"],
                                     grid_size=np.array(GRID), point_cloud_range=np.array(dataset["point_cloud_range"], np.float64),
                                     voxel_size=dataset["voxel_size"], predict_boxes_when_training=False)
        out[name] = {"config": {"MODEL": model_cfg, "dataset": dataset, "grid_size": GRID},
                     "state_dict": shapes(backbone_3d, "backbone_3d.") + shapes(bev, "backbone_2d.") + shapes(dense_head, "dense_head.")}
    write_state_dict("centerpoint_voxel_state_dict.json", out)


if __name__ == "__main__":
    main()
