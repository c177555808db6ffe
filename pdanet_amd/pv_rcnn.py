"""PVRCNN (pcdet/models/detectors/pv_rcnn.py) for kitti_models/pv_rcnn.yaml: MeanVFE -> VoxelBackBone8x -> HeightCompression ->
VoxelSetAbstraction -> BaseBEVBackbone -> AnchorHeadSingle -> PointHeadSimple -> PVRCNNHead, under the reference's module
names and order (vfe, backbone_3d, map_to_bev_module, pfe, backbone_2d, dense_head, point_head, roi_head), so a reference
checkpoint loads with strict=True.  The batch carries `points` (N, 1 + 3 + C) [bs_idx, x, y, z, ...] ordered by scene next to
the voxels.  Training returns ({'loss': loss_rpn + loss_point + loss_rcnn}, tb_dict with the rpn_*, point_* and rcnn_*
entries, disp_dict); eval returns (pred_dicts, recall_dict) with the labels of the first stage's RoIs.

Out of scope: PV-RCNN++ (SPC sampling, VectorPoolAggregationModuleMSG), PointIntraPartOffsetHead."""
from . import model_nms_utils
from .anchor_head import AnchorHeadSingle
from .detector3d_template import VoxelDetector
from .mean_vfe import MeanVFE
from .point_head import PointHeadSimple
from .pvrcnn_head import PVRCNNHead
from .spconv_backbone import VoxelBackBone8x
from .voxel_set_abstraction import VoxelSetAbstraction


class PVRCNN(VoxelDetector):
    VFE = {'MeanVFE': MeanVFE}
    BACKBONE_3D = {'VoxelBackBone8x': VoxelBackBone8x}
    DENSE_HEAD = {'AnchorHeadSingle': AnchorHeadSingle}
    PFE = {'VoxelSetAbstraction': VoxelSetAbstraction}
    POINT_HEAD = {'PointHeadSimple': PointHeadSimple}
    ROI_HEAD = {'PVRCNNHead': PVRCNNHead}

    def __init__(self, model_cfg, num_class, dataset):
        for key in ('PFE', 'POINT_HEAD', 'ROI_HEAD'):
            if model_cfg.get(key, None) is None:
                raise ValueError("PVRCNN needs MODEL.%s" % key)
        super().__init__(model_cfg, num_class, dataset)

    def post_processing(self, batch_dict):
        """(pred_dicts, recall_dict), as VoxelRCNN.post_processing; the scores are the second stage's."""
        cfg = self.model_cfg['POST_PROCESSING']
        padded = model_nms_utils.post_processing(batch_dict, cfg, self.num_class)
        return model_nms_utils.to_pred_and_recall_dicts(padded, cfg.get('RECALL_THRESH_LIST', ()))
