"""VoxelRCNN (pcdet/models/detectors/voxel_rcnn.py) for kitti_models/voxel_rcnn_car.yaml: MeanVFE -> VoxelBackBone8x ->
HeightCompression -> BaseBEVBackbone -> AnchorHeadSingle -> VoxelRCNNHead, under the reference's module names (vfe,
backbone_3d, map_to_bev_module, backbone_2d, dense_head, roi_head), so a reference checkpoint loads with strict=True.
Training returns ({'loss': loss_rpn + loss_rcnn}, tb_dict with the rpn_* and rcnn_* entries, disp_dict); eval returns
(pred_dicts, recall_dict) with the labels of the first stage's RoIs.

Out of scope: the Waymo variant's wiring (CenterHead and DynMeanVFE in front of the same head)."""
from . import model_nms_utils
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

    def __init__(self, model_cfg, num_class, dataset):
        if model_cfg.get('ROI_HEAD', None) is None:
            raise ValueError("VoxelRCNN needs MODEL.ROI_HEAD")
        super().__init__(model_cfg, num_class, dataset)

    def post_processing(self, batch_dict):
        """(pred_dicts, recall_dict), as SECONDNet.post_processing; the scores are the second stage's."""
        cfg = self.model_cfg['POST_PROCESSING']
        padded = model_nms_utils.post_processing(batch_dict, cfg, self.num_class)
        return model_nms_utils.to_pred_and_recall_dicts(padded, cfg.get('RECALL_THRESH_LIST', ()))
