"""CenterPoint (pcdet/models/detectors/centerpoint.py) for the dynamic-pillar configurations of the reference
(centerpoint_dyn_pillar_1x.yaml, cbgs_dyn_pp_centerpoint.yaml): DynPillarVFE -> PointPillarScatter -> BaseBEVBackbone ->
CenterHead, under the reference's module names (vfe, map_to_bev_module, backbone_2d, dense_head), so a reference checkpoint
loads with strict=True.  Training returns ({'loss': loss}, tb_dict, disp_dict) with 0-dim device tensors in tb_dict; eval
returns what model_nms_utils.to_pred_and_recall_dicts returns, after one host read for predictions and recall."""
from . import model_nms_utils
from .center_head import CenterHead
from .detector3d_template import PillarDetector
from .dynamic_vfe import DynamicPillarVFE


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
