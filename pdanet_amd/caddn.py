"""CaDDN (pcdet/models/detectors/caddn.py) for kitti_models/CaDDN.yaml, the camera model of the family: ImageVFE (DepthFFN over
DDNDeepLabV3, FrustumToVoxel) -> Conv2DCollapse -> BaseBEVBackbone -> AnchorHeadSingle, under the reference's module names
(vfe, map_to_bev_module, backbone_2d, dense_head), so a reference checkpoint loads with strict=True.

The batch is the reference's collated one: images (B, 3, H, W) NaN-padded, trans_lidar_to_cam (B, 4, 4), trans_cam_to_img
(B, 3, 4), image_shape (B, 2) [H, W], and for training depth_maps (B, H / f, W / f) NaN-padded, gt_boxes2d (B, N, 4)
zero-padded and gt_boxes (B, M, 8).  The dataset object carries, next to class_names, point_cloud_range, voxel_size and
optionally grid_size, `depth_downsample_factor`; without it the factor is read from the `downsample_depth_map` entry of its
data_processor / DATA_PROCESSOR list.

Training returns ({'loss': loss_rpn + loss_depth}, tb_dict, disp_dict); tb_dict has loss_rpn, loss_depth, the head's rpn_*
entries and DDNLoss's balancer_loss, fg_loss, bg_loss, ddn_loss as 0-dim device tensors.  A forward + loss + backward reads
nothing on the host.  Eval returns what model_nms_utils.to_pred_and_recall_dicts returns.

Out of scope: the image-side data steps (random_image_flip, calculate_grid_size, downsample_depth_map), aux_loss, graph
capture of the ResNet."""
from .anchor_head import AnchorHeadSingle
from .base_bev_backbone import BaseBEVBackbone
from .config import field
from .conv2d_collapse import Conv2DCollapse
from .detector3d_template import PillarDetector, class_count, voxel_geometry
from .image_vfe import ImageVFE


def depth_downsample_factor(dataset):
    """The dataset's own field, or DOWNSAMPLE_FACTOR of the downsample_depth_map step of its processor list."""
    factor = field(dataset, 'depth_downsample_factor', None)
    if factor is not None:
        return factor
    for key in ('DATA_PROCESSOR', 'data_processor'):
        steps = field(dataset, key, None)
        if isinstance(steps, (list, tuple)):
            for step in steps:
                if step.get('NAME') == 'downsample_depth_map':
                    return step['DOWNSAMPLE_FACTOR']
    raise ValueError("CaDDN needs the dataset's depth_downsample_factor (or a downsample_depth_map entry in DATA_PROCESSOR)")


class CaDDN(PillarDetector):
    VFE = {'ImageVFE': ImageVFE}
    MAP_TO_BEV = {'Conv2DCollapse': Conv2DCollapse}
    BACKBONE_2D = {'BaseBEVBackbone': BaseBEVBackbone}
    DENSE_HEAD = {'AnchorHeadSingle': AnchorHeadSingle}
    REQUIRED = ('VFE', 'MAP_TO_BEV', 'BACKBONE_2D', 'DENSE_HEAD')

    def build_modules(self, dataset):
        model_cfg = self.model_cfg
        pcr, vs, grid = voxel_geometry(dataset)
        vfe_cfg, bev_cfg, b2d_cfg, head_cfg = (model_cfg[key] for key in self.REQUIRED)
        self.vfe = self.VFE[vfe_cfg['NAME']](vfe_cfg, grid_size=grid.tolist(), point_cloud_range=pcr.tolist(),
                                             depth_downsample_factor=depth_downsample_factor(dataset))
        self.map_to_bev_module = self.MAP_TO_BEV[bev_cfg['NAME']](bev_cfg, grid_size=grid.tolist())
        self.backbone_2d = BaseBEVBackbone(b2d_cfg, input_channels=self.map_to_bev_module.num_bev_features)
        # the anchors lie on the grid of feature_map_stride (2 in CaDDN.yaml: LAYER_STRIDES [2, 2, 2] against UPSAMPLE_STRIDES
        # [1, 2, 4]); AnchorHeadSingle takes it from ANCHOR_GENERATOR_CONFIG
        self.dense_head = self.DENSE_HEAD[head_cfg['NAME']](
            head_cfg, input_channels=self.backbone_2d.num_bev_features, num_class=class_count(head_cfg, self.num_class),
            class_names=self.class_names, grid_size=grid, point_cloud_range=pcr, voxel_size=vs,
            predict_boxes_when_training=False)
        self.module_list = [self.vfe, self.map_to_bev_module, self.backbone_2d, self.dense_head]

    def get_training_loss(self):
        loss_rpn, tb_dict_rpn = self.dense_head.get_loss()
        loss_depth, tb_dict_depth = self.vfe.get_loss()
        tb_dict = dict({'loss_rpn': loss_rpn.detach(), 'loss_depth': loss_depth.detach()}, **tb_dict_rpn)
        tb_dict.update(tb_dict_depth)
        return loss_rpn + loss_depth, tb_dict, {}


def build(model_cfg, num_class, dataset):
    """The detector of a model config whose NAME is CaDDN."""
    if model_cfg.get('NAME', 'CaDDN') != 'CaDDN':
        raise NotImplementedError("caddn.build: MODEL.NAME %r" % (model_cfg['NAME'],))
    return CaDDN(model_cfg, num_class, dataset)
