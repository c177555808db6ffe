"""VoxelRCNN (pcdet/models/detectors/voxel_rcnn.py) for kitti_models/voxel_rcnn_car.yaml: MeanVFE -> VoxelBackBone8x ->
HeightCompression -> BaseBEVBackbone -> AnchorHeadSingle -> VoxelRCNNHead, under the reference's module names (vfe,
backbone_3d, map_to_bev_module, backbone_2d, dense_head, roi_head), so a reference checkpoint loads with strict=True.
Training returns ({'loss': loss_rpn + loss_rcnn}, tb_dict with the rpn_* and rcnn_* entries, disp_dict); eval returns
(pred_dicts, recall_dict) with the labels of the first stage's RoIs.

Out of scope: the Waymo variant's wiring (CenterHead and DynMeanVFE in front of the same head)."""
from .anchor_head import AnchorHeadSingle
from .detector3d_template import VoxelDetector
from .mean_vfe import MeanVFE
from .spconv_backbone import VoxelBackBone8x
from .voxelrcnn_head import VoxelRCNNHead


class VoxelRCNN(VoxelDetector):
    VFE = {'MeanVFE': MeanVFE}
    BACKBONE_3D = {'VoxelBackBone8x': VoxelBackBone8x}
    DENSE_HEAD = {'AnchorHeadSingle': AnchorHeadSingle}
    ROI_HEAD = {'VoxelRCNNHead': VoxelRCNNHead}
    REQUIRED = ('ROI_HEAD',)
