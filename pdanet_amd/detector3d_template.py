"""What the detectors share (pcdet/models/detectors/detector3d_template.py): the constructor's front -- the dataset fields, the
blocks a detector cannot do without, the check of the NAME keys -- the run over the modules under the reference's module
names, so a reference checkpoint loads with strict=True, the sum of the losses, and post_processing.  A detector names the
classes it accepts per block (VFE, BACKBONE_3D, DENSE_HEAD, PFE, POINT_HEAD, ROI_HEAD: NAME -> class) and the blocks its model
config must have (REQUIRED).  (detector.py, IASSD with its graph capture, does not build on this.)  Three families:

PillarDetector   vfe -> map_to_bev_module (PointPillarScatter) -> backbone_2d -> dense_head: PointPillar, CenterPoint.
VoxelDetector    the sparse-convolution family: vfe -> backbone_3d -> map_to_bev_module (HeightCompression) -> backbone_2d ->
                 dense_head, and -> roi_head for a two-stage detector that names one (ROI_HEAD).  A detector with PFE and
                 POINT_HEAD tables (PV-RCNN) gets pfe after map_to_bev_module and point_head after dense_head, the reference's
                 module order; its batch needs `points` (N, 1 + 3 + C) next to the voxels.  SECONDNet, SECONDNetIoU, VoxelRCNN,
                 PVRCNN.
PointDetector    backbone_3d over the raw points -> point_head -> roi_head: PointRCNN."""
import numpy as np
import torch.nn as nn

from . import model_nms_utils
from .base_bev_backbone import BaseBEVBackbone
from .config import field
from .height_compression import HeightCompression
from .pointpillar_scatter import PointPillarScatter
from .voxel_utils import grid_size as _grid_size


def num_point_features(dataset):
    """The dataset's own field, or the reference's point_feature_encoder.num_point_features."""
    try:
        return field(dataset, 'num_point_features')
    except (KeyError, AttributeError):
        return field(dataset, 'point_feature_encoder').num_point_features


def voxel_geometry(dataset):
    """(point_cloud_range, voxel_size, grid_size) of the dataset as arrays; grid_size from the other two when it has none."""
    pcr = np.asarray(field(dataset, 'point_cloud_range'), dtype=np.float64)
    vs = np.asarray(field(dataset, 'voxel_size'), dtype=np.float64)
    grid = field(dataset, 'grid_size', None)
    return pcr, vs, np.asarray(_grid_size(pcr, vs) if grid is None else grid, dtype=np.int64)


def class_count(cfg, num_class):
    return num_class if not cfg.get('CLASS_AGNOSTIC', False) else 1


class PillarDetector(nn.Module):
    VFE = {}             # NAME -> class, the encoders and heads a detector accepts and builds
    DENSE_HEAD = {}
    REQUIRED = ()        # the blocks of the model config that this detector cannot do without

    def __init__(self, model_cfg, num_class, dataset):
        """dataset: an object or dict with class_names, num_point_features (or the reference's
        point_feature_encoder.num_point_features) and, but for a PointDetector, point_cloud_range, voxel_size and
        optionally grid_size."""
        super().__init__()
        self.model_cfg, self.num_class = model_cfg, num_class
        self.class_names = list(field(dataset, 'class_names'))
        for key in self.REQUIRED:
            self.block(key, getattr(self, key), required=True)
        self.build_modules(dataset)

    def block(self, key, table, required=False):
        """The model config's block `key`, or None when it has none and may; one this detector has no class for is refused."""
        cfg = self.model_cfg.get(key, None)
        if cfg is None:
            if required:
                raise ValueError("%s needs MODEL.%s" % (type(self).__name__, key))
            return None
        if cfg['NAME'] not in table:
            raise NotImplementedError("%s.NAME %r is not part of %s (%s)"
                                      % (key, cfg['NAME'], type(self).__name__, ", ".join(table) or "no such block"))
        return cfg

    def build_modules(self, dataset):
        model_cfg, n_feat = self.model_cfg, num_point_features(dataset)
        pcr, vs, grid = voxel_geometry(dataset)
        # not self.block: the pillar family's refusal keeps its own wording, which tests/test_center_head.py matches whole
        for key, names in (('VFE', self.VFE), ('MAP_TO_BEV', ('PointPillarScatter',)),
                           ('BACKBONE_2D', ('BaseBEVBackbone',)), ('DENSE_HEAD', self.DENSE_HEAD)):
            if model_cfg[key]['NAME'] not in names:
                raise NotImplementedError("%s.NAME %r (the sparse-conv backbones and other heads are not part of this project)"
                                          % (key, model_cfg[key]['NAME']))
        vfe_cfg, head_cfg = model_cfg['VFE'], model_cfg['DENSE_HEAD']
        self.vfe = self.VFE[vfe_cfg['NAME']](vfe_cfg, num_point_features=n_feat, voxel_size=vs, grid_size=grid,
                                             point_cloud_range=pcr)
        self.map_to_bev_module = PointPillarScatter(model_cfg['MAP_TO_BEV'], grid_size=grid)
        self.backbone_2d = BaseBEVBackbone(model_cfg['BACKBONE_2D'], input_channels=self.map_to_bev_module.num_bev_features)
        self.dense_head = self.DENSE_HEAD[head_cfg['NAME']](
            head_cfg, input_channels=self.backbone_2d.num_bev_features, num_class=class_count(head_cfg, self.num_class),
            class_names=self.class_names, grid_size=grid, point_cloud_range=pcr, voxel_size=vs,
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
        """(pred_dicts, recall_dict): model_nms_utils.post_processing on the last head's batch_cls_preds / batch_box_preds
        (a second stage's scores with the labels of the first stage's RoIs), the batch's recall counted on the device when
        gt_boxes is present; one host read for predictions and recall."""
        cfg = self.model_cfg['POST_PROCESSING']
        padded = model_nms_utils.post_processing(batch_dict, cfg, self.num_class)
        return model_nms_utils.to_pred_and_recall_dicts(padded, cfg.get('RECALL_THRESH_LIST', ()))


class VoxelDetector(PillarDetector):
    """The sparse-convolution family: PillarDetector's constructor front, forward and loss over five modules and more."""
    BACKBONE_3D = {}     # NAME -> class
    ROI_HEAD = {}        # NAME -> class; a model config without ROI_HEAD builds the one-stage detector
    PFE = {}             # NAME -> class; built only when the model config has the block (as POINT_HEAD)
    POINT_HEAD = {}

    def build_modules(self, dataset):
        model_cfg, num_class, n_feat = self.model_cfg, self.num_class, num_point_features(dataset)
        pcr, vs, grid = voxel_geometry(dataset)
        vfe_cfg, b3d_cfg, bev_cfg, b2d_cfg, head_cfg = (
            self.block(key, names, required=True) for key, names in (
                ('VFE', self.VFE), ('BACKBONE_3D', self.BACKBONE_3D), ('MAP_TO_BEV', ('HeightCompression',)),
                ('BACKBONE_2D', ('BaseBEVBackbone',)), ('DENSE_HEAD', self.DENSE_HEAD)))
        self.vfe = self.VFE[vfe_cfg['NAME']](vfe_cfg, num_point_features=n_feat, voxel_size=vs, grid_size=grid,
                                             point_cloud_range=pcr)
        self.backbone_3d = self.BACKBONE_3D[b3d_cfg['NAME']](b3d_cfg, input_channels=self.vfe.get_output_feature_dim(),
                                                             grid_size=grid.tolist(), voxel_size=vs, point_cloud_range=pcr)
        self.map_to_bev_module = HeightCompression(bev_cfg, grid_size=grid)
        self.module_list = [self.vfe, self.backbone_3d, self.map_to_bev_module]
        pfe_cfg = self.block('PFE', self.PFE)
        if pfe_cfg is not None:
            self.pfe = self.PFE[pfe_cfg['NAME']](model_cfg=pfe_cfg, voxel_size=vs, point_cloud_range=pcr,
                                                 num_bev_features=self.map_to_bev_module.num_bev_features,
                                                 num_rawpoint_features=n_feat)
            self.module_list.append(self.pfe)
        self.backbone_2d = BaseBEVBackbone(b2d_cfg, input_channels=self.map_to_bev_module.num_bev_features)
        self.dense_head = self.DENSE_HEAD[head_cfg['NAME']](
            head_cfg, input_channels=self.backbone_2d.num_bev_features, num_class=class_count(head_cfg, num_class),
            class_names=self.class_names, grid_size=grid, point_cloud_range=pcr, voxel_size=vs,
            predict_boxes_when_training=model_cfg.get('ROI_HEAD', False))
        self.module_list += [self.backbone_2d, self.dense_head]
        point_cfg = self.block('POINT_HEAD', self.POINT_HEAD)
        if point_cfg is not None:
            if pfe_cfg is None:
                raise ValueError("POINT_HEAD needs a PFE")
            before = point_cfg.get('USE_POINT_FEATURES_BEFORE_FUSION', False)
            self.point_head = self.POINT_HEAD[point_cfg['NAME']](
                model_cfg=point_cfg, input_channels=self.pfe.num_point_features_before_fusion if before else self.pfe.num_point_features,
                num_class=class_count(point_cfg, num_class), predict_boxes_when_training=model_cfg.get('ROI_HEAD', False))
            self.module_list.append(self.point_head)
        roi_cfg = self.block('ROI_HEAD', self.ROI_HEAD)
        if roi_cfg is not None:
            point_kwargs = {} if pfe_cfg is None else {'input_channels': self.pfe.num_point_features}
            self.roi_head = self.ROI_HEAD[roi_cfg['NAME']](
                backbone_channels=self.backbone_3d.backbone_channels, model_cfg=roi_cfg, point_cloud_range=pcr, voxel_size=vs,
                num_class=class_count(roi_cfg, num_class), **point_kwargs)
            self.module_list.append(self.roi_head)

    def forward(self, batch_dict):
        """A padded batch (voxel_num_active, voxel_utils.collate_voxels_padded) runs the one-stage detectors without a host
        read; the voxel queries and RoI pools of a second stage are not count-aware and refuse it."""
        if batch_dict.get('voxel_num_active') is not None and any(
                getattr(self, name, None) is not None for name in ('pfe', 'point_head', 'roi_head')):
            raise NotImplementedError("%s: a padded batch (voxel_num_active) is implemented for the one-stage detectors only; "
                                      "the second stage's voxel queries and RoI pools are not count-aware" % type(self).__name__)
        return super().forward(batch_dict)

    def get_training_loss(self):
        loss, tb_dict, disp_dict = super().get_training_loss()
        if getattr(self, 'point_head', None) is not None:
            loss_point, tb_dict = self.point_head.get_loss(tb_dict)
            loss = loss + loss_point
        if getattr(self, 'roi_head', None) is not None:
            loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
            loss = loss + loss_rcnn
        return loss, tb_dict, disp_dict


class PointDetector(PillarDetector):
    """The point-based family: backbone_3d over the raw points -> point_head -> roi_head, the reference's module order for
    PointRCNN.  No voxels, no BEV map, no dense head, and nothing of the dataset's geometry.  The batch carries `points`
    (N, 1 + 3 + C) [bs_idx, x, y, z, ...] ordered by scene with equally many rows per scene."""
    BACKBONE_3D = {}     # NAME -> class
    POINT_HEAD = {}
    ROI_HEAD = {}        # a model config without ROI_HEAD builds the one-stage detector
    REQUIRED = ('BACKBONE_3D', 'POINT_HEAD')

    def build_modules(self, dataset):
        model_cfg, num_class = self.model_cfg, self.num_class
        b3d_cfg, point_cfg = model_cfg['BACKBONE_3D'], model_cfg['POINT_HEAD']
        self.backbone_3d = self.BACKBONE_3D[b3d_cfg['NAME']](model_cfg=b3d_cfg, input_channels=num_point_features(dataset))
        n_point = self.backbone_3d.num_point_features
        self.point_head = self.POINT_HEAD[point_cfg['NAME']](
            model_cfg=point_cfg, input_channels=n_point, num_class=class_count(point_cfg, num_class),
            predict_boxes_when_training=model_cfg.get('ROI_HEAD', False))
        self.module_list = [self.backbone_3d, self.point_head]
        roi_cfg = self.block('ROI_HEAD', self.ROI_HEAD)
        if roi_cfg is not None:
            self.roi_head = self.ROI_HEAD[roi_cfg['NAME']](model_cfg=roi_cfg, input_channels=n_point,
                                                           num_class=class_count(roi_cfg, num_class))
            self.module_list.append(self.roi_head)

    def get_training_loss(self):
        loss_point, tb_dict = self.point_head.get_loss()
        loss = loss_point
        if getattr(self, 'roi_head', None) is not None:
            loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
            loss = loss + loss_rcnn
        return loss, tb_dict, {}
