"""PointPillar (pcdet/models/detectors/pointpillar.py) for kitti_models/pointpillar.yaml, pointpillar_newaugs.yaml and
waymo_models/pointpillar_1x.yaml: PillarVFE -> PointPillarScatter -> BaseBEVBackbone -> AnchorHeadSingle, under the
reference's module names (vfe, map_to_bev_module, backbone_2d, dense_head), so a reference checkpoint loads with
strict=True.  The batch carries the collated hard voxels (voxel_utils.VoxelGenerator.generate_batch + collate_voxels).
Training returns ({'loss': loss}, tb_dict, disp_dict) with 0-dim device tensors in tb_dict; eval returns what
model_nms_utils.to_pred_and_recall_dicts returns, after one host read for predictions and recall."""
import numpy as np
import torch.nn as nn

from . import model_nms_utils
from .anchor_head import AnchorHeadSingle
from .base_bev_backbone import BaseBEVBackbone
from .centerpoint import _field
from .pillar_vfe import PillarVFE
from .pointpillar_scatter import PointPillarScatter
from .voxel_utils import grid_size as _grid_size


class PointPillar(nn.Module):
    def __init__(self, model_cfg, num_class, dataset):
        """dataset: an object or dict with class_names, point_cloud_range, voxel_size, num_point_features (or the
        reference's point_feature_encoder.num_point_features) and optionally grid_size."""
        super().__init__()
        self.model_cfg, self.num_class = model_cfg, num_class
        self.class_names = list(_field(dataset, 'class_names'))
        pcr = np.asarray(_field(dataset, 'point_cloud_range'), dtype=np.float64)
        vs = np.asarray(_field(dataset, 'voxel_size'), dtype=np.float64)
        try:
            grid = _field(dataset, 'grid_size')
        except (KeyError, AttributeError):
            grid = None
        grid = np.asarray(_grid_size(pcr, vs) if grid is None else grid, dtype=np.int64)
        try:
            n_feat = _field(dataset, 'num_point_features')
        except (KeyError, AttributeError):
            n_feat = _field(dataset, 'point_feature_encoder').num_point_features
        for key, names in (('VFE', ('PillarVFE',)), ('MAP_TO_BEV', ('PointPillarScatter',)),
                           ('BACKBONE_2D', ('BaseBEVBackbone',)), ('DENSE_HEAD', ('AnchorHeadSingle',))):
            if model_cfg[key]['NAME'] not in names:
                raise NotImplementedError("%s.NAME %r (the sparse-conv backbones and other heads are not part of this project)"
                                          % (key, model_cfg[key]['NAME']))
        self.vfe = PillarVFE(model_cfg['VFE'], num_point_features=n_feat, voxel_size=vs, point_cloud_range=pcr)
        self.map_to_bev_module = PointPillarScatter(model_cfg['MAP_TO_BEV'], grid_size=grid)
        self.backbone_2d = BaseBEVBackbone(model_cfg['BACKBONE_2D'], input_channels=self.map_to_bev_module.num_bev_features)
        self.dense_head = AnchorHeadSingle(model_cfg['DENSE_HEAD'], input_channels=self.backbone_2d.num_bev_features,
                                           num_class=num_class if not model_cfg['DENSE_HEAD'].get('CLASS_AGNOSTIC', False) else 1,
                                           class_names=self.class_names, grid_size=grid, point_cloud_range=pcr,
                                           predict_boxes_when_training=model_cfg.get('ROI_HEAD', False))
        self.module_list = [self.vfe, self.map_to_bev_module, self.backbone_2d, self.dense_head]

    def forward(self, batch_dict):
        for module in self.module_list:
            batch_dict = module(batch_dict)
        if self.training:
            loss, tb_dict, disp_dict = self.get_training_loss()
            return {'loss': loss}, tb_dict, disp_dict
        return self.post_processing(batch_dict)

    def get_training_loss(self):
        loss_rpn, tb_dict = self.dense_head.get_loss()
        return loss_rpn, dict({'loss_rpn': loss_rpn.detach()}, **tb_dict), {}

    def post_processing(self, batch_dict):
        """(pred_dicts, recall_dict): model_nms_utils.post_processing on the head's batch_cls_preds / batch_box_preds, the
        batch's recall counted on the device when gt_boxes is present."""
        cfg = self.model_cfg['POST_PROCESSING']
        padded = model_nms_utils.post_processing(batch_dict, cfg, self.num_class)
        return model_nms_utils.to_pred_and_recall_dicts(padded, cfg.get('RECALL_THRESH_LIST', ()))
