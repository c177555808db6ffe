"""PartA2Net (pcdet/models/detectors/PartA2_net.py) for kitti_models/PartA2.yaml and waymo_models/PartA2.yaml: MeanVFE -> UNetV2
-> HeightCompression -> BaseBEVBackbone -> AnchorHeadSingle -> PointIntraPartOffsetHead -> PartA2FCHead, under the reference's
module names and order (vfe, backbone_3d, map_to_bev_module, backbone_2d, dense_head, point_head, roi_head), so a reference
checkpoint loads with strict=True.  UNetV2 hands the point head its voxel centres and their features, so there is no PFE and
the batch needs no raw points.  Training returns ({'loss': loss_rpn + loss_point + loss_rcnn}, tb_dict with the rpn_*, point_*
and rcnn_* entries, disp_dict); eval returns (pred_dicts, recall_dict) with the labels of the first stage's RoIs.

Host reads of a training iteration: the four strided rulebook builds of UNetV2 and the live-voxel count of the RoI head's input
stage.

Out of scope: the anchor-free kitti_models/PartA2_free.yaml, which has no DENSE_HEAD -- PointIntraPartOffsetHead proposes the
boxes there (TARGET_CONFIG.BOX_CODER), PartA2FCHead is the same; a model config without DENSE_HEAD is refused by name."""
from .anchor_head import AnchorHeadSingle
from .detector3d_template import VoxelDetector, class_count
from .mean_vfe import MeanVFE
from .part_head import PointIntraPartOffsetHead
from .parta2_head import PartA2FCHead
from .spconv_unet import UNetV2


class PartA2Net(VoxelDetector):
    VFE = {'MeanVFE': MeanVFE}
    BACKBONE_3D = {'UNetV2': UNetV2}
    DENSE_HEAD = {'AnchorHeadSingle': AnchorHeadSingle}
    # the second stage, built here: VoxelDetector.build_modules gives a point head a PFE's features and a RoI head the
    # backbone's multi-scale channels, and this detector has neither
    POINT_HEADS = {'PointIntraPartOffsetHead': PointIntraPartOffsetHead}
    ROI_HEADS = {'PartA2FCHead': PartA2FCHead}

    def build_modules(self, dataset):
        full = self.model_cfg
        if full.get('DENSE_HEAD', None) is None:
            raise NotImplementedError("PartA2Net without MODEL.DENSE_HEAD (the anchor-free PartA2_free.yaml, where the point head "
                                      "proposes the boxes) is not implemented")
        if full.get('PFE', None) is not None:
            raise NotImplementedError("PFE.NAME %r is not part of PartA2Net (no such block)" % (full['PFE']['NAME'],))
        point_cfg = self.block('POINT_HEAD', self.POINT_HEADS, required=True)
        roi_cfg = self.block('ROI_HEAD', self.ROI_HEADS, required=True)
        # the first stage, from the config without the two blocks
        self.model_cfg = type(full)((k, v) for k, v in full.items() if k not in ('POINT_HEAD', 'ROI_HEAD'))
        try:
            super().build_modules(dataset)
        finally:
            self.model_cfg = full
        self.dense_head.predict_boxes_when_training = True          # what MODEL.ROI_HEAD means to the first stage
        n_point = self.backbone_3d.num_point_features
        self.point_head = self.POINT_HEADS[point_cfg['NAME']](model_cfg=point_cfg, input_channels=n_point,
                                                              num_class=class_count(point_cfg, self.num_class),
                                                              predict_boxes_when_training=True)
        self.roi_head = self.ROI_HEADS[roi_cfg['NAME']](model_cfg=roi_cfg, input_channels=n_point,
                                                        num_class=class_count(roi_cfg, self.num_class))
        self.module_list += [self.point_head, self.roi_head]
