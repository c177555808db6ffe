"""SECONDNetIoU (pcdet/models/detectors/second_net_iou.py) for kitti_models/second_iou.yaml: MeanVFE -> VoxelBackBone8x ->
HeightCompression -> BaseBEVBackbone -> AnchorHeadSingle -> SECONDHead, under the reference's module names (vfe,
backbone_3d, map_to_bev_module, backbone_2d, dense_head, roi_head), so a reference checkpoint loads with strict=True.
Training returns ({'loss': loss_rpn + loss_rcnn}, tb_dict with the rpn_* and rcnn_* entries, disp_dict); eval re-scores the
RoIs from the IoU branch and the first stage's score (POST_PROCESSING.NMS_CONFIG.SCORE_TYPE) and returns
(pred_dicts, recall_dict), the pred dicts with pred_cls_scores and pred_iou_scores next to the three usual keys.

The geometry reaches the head through its constructor, so forward() does not put dataset_cfg into the batch.  The score
type num_pts_iou_cls needs batch_dict['points'] (N, 1 + 3 + C) next to the voxels."""
from . import model_nms_utils
from .anchor_head import AnchorHeadSingle
from .detector3d_template import VoxelDetector
from .mean_vfe import MeanVFE
from .second_head import SECONDHead
from .spconv_backbone import VoxelBackBone8x, VoxelResBackBone8x


class SECONDNetIoU(VoxelDetector):
    VFE = {'MeanVFE': MeanVFE}
    BACKBONE_3D = {'VoxelBackBone8x': VoxelBackBone8x, 'VoxelResBackBone8x': VoxelResBackBone8x}
    DENSE_HEAD = {'AnchorHeadSingle': AnchorHeadSingle}
    ROI_HEAD = {'SECONDHead': SECONDHead}
    REQUIRED = ('ROI_HEAD',)

    def __init__(self, model_cfg, num_class, dataset):
        if model_cfg['POST_PROCESSING']['NMS_CONFIG']['MULTI_CLASSES_NMS']:
            raise NotImplementedError("POST_PROCESSING.NMS_CONFIG.MULTI_CLASSES_NMS")
        super().__init__(model_cfg, num_class, dataset)

    def post_processing(self, batch_dict):
        """(pred_dicts, recall_dict); model_nms_utils.post_processing_iou keeps everything on the device until the one read."""
        cfg = self.model_cfg['POST_PROCESSING']
        padded = model_nms_utils.post_processing_iou(batch_dict, cfg, self.num_class, self.class_names)
        return model_nms_utils.to_iou_pred_and_recall_dicts(padded, cfg.get('RECALL_THRESH_LIST', ()))
