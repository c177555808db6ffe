"""VoxelRCNN (pcdet/models/detectors/voxel_rcnn.py) for kitti_models/voxel_rcnn_car.yaml -- MeanVFE -> VoxelBackBone8x ->
HeightCompression -> BaseBEVBackbone -> AnchorHeadSingle -> VoxelRCNNHead -- and for
waymo_models/voxel_rcnn_with_centerhead_dyn_voxel.yaml, with DynMeanVFE in front (the batch then carries `points` only and the
encoder makes its one host read) and CenterHead as the first stage, under the reference's module names (vfe, backbone_3d,
map_to_bev_module, backbone_2d, dense_head, roi_head), so a reference checkpoint loads with strict=True.
Training returns ({'loss': loss_rpn + loss_rcnn}, tb_dict with the rpn_* and rcnn_* entries, disp_dict); eval returns
(pred_dicts, recall_dict) with the labels of the first stage's RoIs.

CenterHead as the first stage: the head leaves its padded rois / roi_scores / roi_labels (0 = padding) with has_class_labels
in the batch, proposal_layer returns early on them, and they go into assign_targets and the pool as they are."""
from .anchor_head import AnchorHeadSingle
from .center_head import CenterHead
from .detector3d_template import VoxelDetector
from .dynamic_vfe import DynamicMeanVFE
from .mean_vfe import MeanVFE
from .spconv_backbone import VoxelBackBone8x
from .voxelrcnn_head import VoxelRCNNHead


class VoxelRCNN(VoxelDetector):
    VFE = {'MeanVFE': MeanVFE, 'DynMeanVFE': DynamicMeanVFE, 'DynamicMeanVFE': DynamicMeanVFE}
    BACKBONE_3D = {'VoxelBackBone8x': VoxelBackBone8x}
    DENSE_HEAD = {'AnchorHeadSingle': AnchorHeadSingle, 'CenterHead': CenterHead}
    ROI_HEAD = {'VoxelRCNNHead': VoxelRCNNHead}
    REQUIRED = ('ROI_HEAD',)
