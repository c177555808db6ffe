"""PointPillar (pcdet/models/detectors/pointpillar.py) for kitti_models/pointpillar.yaml, pointpillar_newaugs.yaml and
waymo_models/pointpillar_1x.yaml: PillarVFE -> PointPillarScatter -> BaseBEVBackbone -> AnchorHeadSingle, under the
reference's module names (vfe, map_to_bev_module, backbone_2d, dense_head), so a reference checkpoint loads with
strict=True.  The batch carries the collated hard voxels (voxel_utils.VoxelGenerator.generate_batch + collate_voxels).
Training returns ({'loss': loss}, tb_dict, disp_dict) with 0-dim device tensors in tb_dict; eval returns what
model_nms_utils.to_pred_and_recall_dicts returns, after one host read for predictions and recall."""
from . import model_nms_utils
from .anchor_head import AnchorHeadSingle
from .detector3d_template import PillarDetector
from .pillar_vfe import PillarVFE


class PointPillar(PillarDetector):
    VFE = {'PillarVFE': PillarVFE}
    DENSE_HEAD = {'AnchorHeadSingle': AnchorHeadSingle}

    def post_processing(self, batch_dict):
        """(pred_dicts, recall_dict): model_nms_utils.post_processing on the head's batch_cls_preds / batch_box_preds, the
        batch's recall counted on the device when gt_boxes is present."""
        cfg = self.model_cfg['POST_PROCESSING']
        padded = model_nms_utils.post_processing(batch_dict, cfg, self.num_class)
        return model_nms_utils.to_pred_and_recall_dicts(padded, cfg.get('RECALL_THRESH_LIST', ()))
