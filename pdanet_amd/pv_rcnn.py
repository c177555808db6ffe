"""PVRCNN (pcdet/models/detectors/pv_rcnn.py) for kitti_models/pv_rcnn.yaml: MeanVFE -> VoxelBackBone8x -> HeightCompression ->
VoxelSetAbstraction -> BaseBEVBackbone -> AnchorHeadSingle -> PointHeadSimple -> PVRCNNHead, under the reference's module
names and order (vfe, backbone_3d, map_to_bev_module, pfe, backbone_2d, dense_head, point_head, roi_head), so a reference
checkpoint loads with strict=True.  The batch carries `points` (N, 1 + 3 + C) [bs_idx, x, y, z, ...] ordered by scene next to
the voxels.  Training returns ({'loss': loss_rpn + loss_point + loss_rcnn}, tb_dict with the rpn_*, point_* and rcnn_*
entries, disp_dict); eval returns (pred_dicts, recall_dict) with the labels of the first stage's RoIs.
waymo_models/pv_rcnn_with_centerhead_rpn.yaml: CenterHead as the first stage, whose padded rois / roi_scores / roi_labels
pass proposal_layer's early return (voxel_rcnn.py).

Out of scope: PV-RCNN++ (SPC sampling, VectorPoolAggregationModuleMSG); PointIntraPartOffsetHead belongs to PartA2Net."""
from .anchor_head import AnchorHeadSingle
from .center_head import CenterHead
from .detector3d_template import VoxelDetector
from .mean_vfe import MeanVFE
from .point_head import PointHeadSimple
from .pvrcnn_head import PVRCNNHead
from .spconv_backbone import VoxelBackBone8x
from .voxel_set_abstraction import VoxelSetAbstraction


class PVRCNN(VoxelDetector):
    VFE = {'MeanVFE': MeanVFE}
    BACKBONE_3D = {'VoxelBackBone8x': VoxelBackBone8x}
    DENSE_HEAD = {'AnchorHeadSingle': AnchorHeadSingle, 'CenterHead': CenterHead}
    PFE = {'VoxelSetAbstraction': VoxelSetAbstraction}
    POINT_HEAD = {'PointHeadSimple': PointHeadSimple}
    ROI_HEAD = {'PVRCNNHead': PVRCNNHead}
    REQUIRED = ('PFE', 'POINT_HEAD', 'ROI_HEAD')
