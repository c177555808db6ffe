"""CenterPoint (pcdet/models/detectors/centerpoint.py), which the reference builds under one NAME for two families:

CenterPoint        the dynamic-pillar configurations (centerpoint_dyn_pillar_1x.yaml, cbgs_dyn_pp_centerpoint.yaml):
                   DynPillarVFE -> PointPillarScatter -> BaseBEVBackbone -> CenterHead, under the reference's module names
                   (vfe, map_to_bev_module, backbone_2d, dense_head).
VoxelCenterPoint   the voxel configurations (kitti_models/centerpoint.yaml, waymo_models/centerpoint.yaml and
                   centerpoint_without_resnet.yaml, nuscenes_models/cbgs_voxel0075_res3d_centerpoint.yaml and
                   cbgs_voxel01_res3d_centerpoint.yaml): MeanVFE / DynMeanVFE -> VoxelBackBone8x / VoxelResBackBone8x ->
                   HeightCompression -> BaseBEVBackbone -> CenterHead (vfe, backbone_3d, map_to_bev_module, backbone_2d,
                   dense_head).  A padded batch (voxel_num_active, voxel_utils.collate_voxels_padded; MeanVFE only) runs
                   forward, loss and backward without a host read and replays from one captured graph.

A reference checkpoint (spconv 2.x layout) loads into either with strict=True.  Training returns ({'loss': loss}, tb_dict,
disp_dict) with 0-dim device tensors in tb_dict; eval returns what model_nms_utils.to_pred_and_recall_dicts returns, after one
host read for predictions and recall.  build() picks the class as the reference's one NAME does: by BACKBONE_3D."""
from . import model_nms_utils
from .center_head import CenterHead
from .detector3d_template import PillarDetector, VoxelDetector
from .dynamic_vfe import DynamicMeanVFE, DynamicPillarVFE
from .mean_vfe import MeanVFE
from .spconv_backbone import VoxelBackBone8x, VoxelResBackBone8x


class CenterPoint(PillarDetector):
    VFE = {'DynPillarVFE': DynamicPillarVFE, 'DynamicPillarVFE': DynamicPillarVFE}
    DENSE_HEAD = {'CenterHead': CenterHead}

    def post_processing(self, batch_dict):
        """(pred_dicts, recall_dict): the head's padded boxes, with the batch's recall counted on the device when gt_boxes
        is present and RECALL_MODE is 'normal' (the default)."""
        cfg = self.model_cfg['POST_PROCESSING']
        padded = batch_dict['final_padded']
        thresh = cfg.get('RECALL_THRESH_LIST', ())
        if cfg.get('RECALL_MODE', 'normal') == 'normal' and 'gt_boxes' in batch_dict and len(thresh):
            padded['recall'] = model_nms_utils.recall_record(padded['pred_boxes'], padded['num_pred'], batch_dict['gt_boxes'], thresh)
        return model_nms_utils.to_pred_and_recall_dicts(padded, thresh)


class VoxelCenterPoint(VoxelDetector):
    VFE = {'MeanVFE': MeanVFE, 'DynMeanVFE': DynamicMeanVFE, 'DynamicMeanVFE': DynamicMeanVFE}
    BACKBONE_3D = {'VoxelBackBone8x': VoxelBackBone8x, 'VoxelResBackBone8x': VoxelResBackBone8x}
    DENSE_HEAD = {'CenterHead': CenterHead}
    post_processing = CenterPoint.post_processing          # the head leaves final_padded: one function for both families

    def forward(self, batch_dict):
        if batch_dict.get('voxel_num_active') is not None and not isinstance(self.vfe, MeanVFE):
            raise NotImplementedError("VoxelCenterPoint: a padded batch (voxel_num_active) carries the hard voxels that MeanVFE "
                                      "takes; %s makes its voxels from `points` and reads their count" % type(self.vfe).__name__)
        return super().forward(batch_dict)


def build(model_cfg, num_class, dataset):
    """The detector of a model config whose NAME is CenterPoint: VoxelCenterPoint when it has a BACKBONE_3D, CenterPoint (the
    pillars) otherwise."""
    cls = VoxelCenterPoint if model_cfg.get('BACKBONE_3D', None) is not None else CenterPoint
    return cls(model_cfg, num_class, dataset)
