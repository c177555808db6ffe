"""PVRCNNPlusPlus (pcdet/models/detectors/pv_rcnn_plusplus.py) for waymo_models/pv_rcnn_plusplus.yaml and
pv_rcnn_plusplus_resnet.yaml: MeanVFE -> VoxelBackBone8x | VoxelResBackBone8x -> HeightCompression -> BaseBEVBackbone ->
CenterHead, then the proposals, and only then VoxelSetAbstraction (SPC keypoints, RoI-filtered sources, VectorPool layers:
voxel_set_abstraction_spc.py, vector_pool_modules.py) -> PointHeadSimple (its targets assigned over ragged keypoints) ->
PVRCNNHead with a VectorPool RoI-grid pool.  The
modules are registered under the reference's names in the reference's order (vfe, backbone_3d, map_to_bev_module, pfe,
backbone_2d, dense_head, point_head, roi_head), so a reference checkpoint loads with strict=True; they RUN in the order of the
reference's forward, because the keypoints and the source filters need the RoIs.

In training the sampled targets are made before the keypoint encoder and handed to the head as batch_dict['roi_targets_dict']
(PVRCNNHead.forward takes them as they are); batch_dict may carry 'roi_target_seed' / 'roi_target_draws'.
Training returns ({'loss': loss_rpn + loss_point + loss_rcnn}, tb_dict, disp_dict); eval returns (pred_dicts, recall_dict).

Refused with NotImplementedError: POINT_SOURCE other than raw_points / voxel_centers (by VoxelSetAbstraction), a padded batch
(voxel_num_active: the second stage is not count-aware), graph capture of the forward (the keypoint encoder and the VectorPool
layers read counts on the host)."""
import torch

from . import vector_pool_modules
from .center_head import CenterHead
from .detector3d_template import VoxelDetector
from .mean_vfe import MeanVFE
from .part_head import part_assign_targets
from .point_head import PointHeadSimple
from .pvrcnn_head import PVRCNNHead
from .spconv_backbone import VoxelBackBone8x, VoxelResBackBone8x
from .voxel_set_abstraction_spc import VoxelSetAbstractionSPC


class PVRCNNPlusPlusHead(PVRCNNHead):
    """PVRCNNHead whose ROI_GRID_POOL may name VectorPoolAggregationModuleMSG."""
    build_local_aggregation_module = staticmethod(vector_pool_modules.build_local_aggregation_module)


class RaggedPointHeadSimple(PointHeadSimple):
    """PointHeadSimple over SPC's keypoints, whose number differs from scene to scene: the labels come from
    part_head.part_assign_targets (csrc/parta2.hip), the same box test, ignore band and classes for a ragged stacked point set
    in one launch; PointHeadTemplate's own launch derives a point's scene from its row and needs equally many rows per scene."""

    def assign_stack_targets(self, points, gt_boxes, extend_gt_boxes=None, ret_box_labels=False, ret_part_labels=False,
                             set_ignore_flag=True, use_ball_constraint=False, central_radius=2.0, extra_width=(0.0, 0.0, 0.0)):
        if ret_box_labels or ret_part_labels or use_ball_constraint or not set_ignore_flag:
            raise NotImplementedError("RaggedPointHeadSimple assigns class labels with the ignore band only")
        labels, _ = part_assign_targets(points.detach().float().contiguous(), gt_boxes.detach().float().contiguous(), extra_width,
                                        self.num_class == 1)
        return {'point_cls_labels': labels, 'point_box_labels': None, 'point_part_labels': None}


class PVRCNNPlusPlus(VoxelDetector):
    VFE = {'MeanVFE': MeanVFE}
    BACKBONE_3D = {'VoxelBackBone8x': VoxelBackBone8x, 'VoxelResBackBone8x': VoxelResBackBone8x}
    DENSE_HEAD = {'CenterHead': CenterHead}
    PFE = {'VoxelSetAbstraction': VoxelSetAbstractionSPC}
    POINT_HEAD = {'PointHeadSimple': RaggedPointHeadSimple}
    ROI_HEAD = {'PVRCNNHead': PVRCNNPlusPlusHead}
    REQUIRED = ('PFE', 'POINT_HEAD', 'ROI_HEAD')

    def forward(self, batch_dict):
        if batch_dict.get('voxel_num_active') is not None:
            raise NotImplementedError("PVRCNNPlusPlus: a padded batch (voxel_num_active) is implemented for the one-stage "
                                      "detectors only; the second stage's filters and pools are not count-aware")
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("PVRCNNPlusPlus: graph capture (the keypoint sampling, the source filters and the "
                                      "VectorPool layers read counts on the host)")
        for module in (self.vfe, self.backbone_3d, self.map_to_bev_module, self.backbone_2d, self.dense_head):
            batch_dict = module(batch_dict)
        targets_dict = self.roi_head.proposals_and_targets(batch_dict)
        if self.training:
            batch_dict['roi_targets_dict'] = targets_dict
        for module in (self.pfe, self.point_head, self.roi_head):
            batch_dict = module(batch_dict)
        if self.training:
            loss, tb_dict, disp_dict = self.get_training_loss()
            return {'loss': loss}, tb_dict, disp_dict
        return self.post_processing(batch_dict)

    def get_training_loss(self):
        loss_rpn, tb_dict = self.dense_head.get_loss()
        loss_point, tb_dict = self.point_head.get_loss(tb_dict)
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
        return loss_rpn + loss_point + loss_rcnn, tb_dict, {}


def build(model_cfg, num_class, dataset):
    """The detector of a model config whose NAME is PVRCNNPlusPlus."""
    if model_cfg.get('NAME', 'PVRCNNPlusPlus') != 'PVRCNNPlusPlus':
        raise NotImplementedError("pv_rcnn_plusplus.build: MODEL.NAME %r" % (model_cfg['NAME'],))
    return PVRCNNPlusPlus(model_cfg, num_class, dataset)
