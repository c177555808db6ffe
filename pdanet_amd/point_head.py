"""PointHeadTemplate, PointHeadSimple and PointHeadBox (pcdet/models/dense_heads/point_head_template.py, point_head_simple.py,
point_head_box.py): the keypoint segmentation head of PV-RCNN and the first stage of PointRCNN, under the reference's module
names (cls_layers, box_layers) and state-dict keys.

assign_stack_targets labels the keypoints of the whole batch in one launch (roiaware_pool3d_utils.head_assign_targets,
csrc/head_targets.hip, mode 0: foreground = inside a ground-truth box, ignored = inside the enlarged box only), where the
reference loops over the scenes with boolean masks and two points_in_boxes_gpu calls each; nothing is read on the host.  The
points must be scene-major with equally many rows per scene, as VoxelSetAbstraction leaves its keypoints.

With ret_box_labels the labels and each point's box come from that same launch; box_coder.encode_torch then runs on all rows
and the rows whose label is <= 0 are zeroed, where the reference encodes the foreground subset it took with a boolean mask.

The one departure from the reference: tb_dict values (point_loss_cls, point_loss_box, point_pos_num) stay 0-dim device tensors
where the reference calls .item().  The per-point loss terms are added in float64 (one deterministic torch reduction) and the sum is
rounded to float32 once, as this project's loss kernels do (csrc/loss_sums.h); the reference adds them in float32.

Refused here (NotImplementedError): ret_part_labels, use_ball_constraint -- PointHeadSimple and PointHeadBox need neither;
PointIntraPartOffsetHead (part_head.py) assigns its part labels with a kernel of its own."""
import torch
import torch.nn as nn

from . import box_coder_utils, loss_utils
from .roiaware_pool3d_utils import head_assign_targets


class PointHeadTemplate(nn.Module):
    def __init__(self, model_cfg, num_class):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.build_losses(model_cfg['LOSS_CONFIG'])
        self.forward_ret_dict = None

    def build_losses(self, losses_cfg):
        self.add_module('cls_loss_func', loss_utils.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0))
        # (the reference's other LOSS_REG choices are torch functionals that get_box_layer_loss's `weights=` call cannot take)
        self.reg_loss_func = None
        if losses_cfg.get('LOSS_REG', None) == 'WeightedSmoothL1Loss':
            self.reg_loss_func = loss_utils.WeightedSmoothL1Loss(code_weights=losses_cfg['LOSS_WEIGHTS'].get('code_weights', None))

    @staticmethod
    def make_fc_layers(fc_cfg, input_channels, output_channels):
        fc_layers = []
        c_in = input_channels
        for k in range(len(fc_cfg)):
            fc_layers.extend([nn.Linear(c_in, fc_cfg[k], bias=False), nn.BatchNorm1d(fc_cfg[k]), nn.ReLU()])
            c_in = fc_cfg[k]
        fc_layers.append(nn.Linear(c_in, output_channels, bias=True))
        return nn.Sequential(*fc_layers)

    def assign_stack_targets(self, points, gt_boxes, extend_gt_boxes=None, ret_box_labels=False, ret_part_labels=False,
                             set_ignore_flag=True, use_ball_constraint=False, central_radius=2.0, extra_width=(0.0, 0.0, 0.0)):
        """points (B * N, 4) [bs_idx, x, y, z] scene-major, gt_boxes (B, M, 8) -> point_cls_labels (B * N) int64: 0 background,
        -1 ignored, else 1 (num_class 1) or the class of the box; with ret_box_labels also point_box_labels (B * N, 8), the
        codes of each foreground point's box against the point and zero elsewhere.  The enlarged boxes are made by the kernel
        from `extra_width`; `extend_gt_boxes` is accepted for the reference's signature and not read."""
        assert points.dim() == 2 and points.shape[1] == 4, 'points.shape=%s' % str(points.shape)
        assert gt_boxes.dim() == 3 and gt_boxes.shape[2] == 8, 'gt_boxes.shape=%s' % str(gt_boxes.shape)
        if ret_part_labels or use_ball_constraint or not set_ignore_flag:
            raise NotImplementedError("ret_part_labels / use_ball_constraint are not part of this project")
        batch_size = gt_boxes.shape[0]
        if points.shape[0] % batch_size != 0:
            raise ValueError("assign_stack_targets needs equally many points per scene, got %d rows for %d scenes"
                             % (points.shape[0], batch_size))
        points = points.detach().float().contiguous()
        labels, _, gt_of_points, _ = head_assign_targets(points, gt_boxes.detach().float().contiguous(), extra_width, 0,
                                                         self.num_class == 1)
        box_labels = None
        if ret_box_labels:
            # a background row carries whatever box index -1 wrapped to: its class is brought into the coder's range and its
            # codes are dropped
            classes = gt_of_points[:, 7].long()
            if getattr(self.box_coder, 'use_mean_size', False):
                classes = classes.clamp(min=1, max=self.box_coder.mean_size.shape[0])
            codes = self.box_coder.encode_torch(gt_boxes=gt_of_points[:, 0:7], points=points[:, 1:4], gt_classes=classes)
            box_labels = torch.where((labels > 0).unsqueeze(-1), codes, torch.zeros_like(codes))
        return {'point_cls_labels': labels, 'point_box_labels': box_labels, 'point_part_labels': None}

    def get_cls_layer_loss(self, tb_dict=None):
        point_cls_labels = self.forward_ret_dict['point_cls_labels'].view(-1)
        point_cls_preds = self.forward_ret_dict['point_cls_preds'].view(-1, self.num_class)

        positives = (point_cls_labels > 0)
        negative_cls_weights = (point_cls_labels == 0) * 1.0
        cls_weights = (negative_cls_weights + 1.0 * positives).float()
        pos_normalizer = positives.sum(dim=0).float()
        cls_weights = cls_weights / torch.clamp(pos_normalizer, min=1.0)

        one_hot_targets = point_cls_preds.new_zeros(*list(point_cls_labels.shape), self.num_class + 1)
        one_hot_targets.scatter_(-1, (point_cls_labels * (point_cls_labels >= 0).long()).unsqueeze(dim=-1).long(), 1.0)
        one_hot_targets = one_hot_targets[..., 1:]
        cls_loss_src = self.cls_loss_func(point_cls_preds, one_hot_targets, weights=cls_weights)
        point_loss_cls = cls_loss_src.sum(dtype=torch.float64).to(cls_loss_src.dtype)

        point_loss_cls = point_loss_cls * self.model_cfg['LOSS_CONFIG']['LOSS_WEIGHTS']['point_cls_weight']
        if tb_dict is None:
            tb_dict = {}
        tb_dict.update({'point_loss_cls': point_loss_cls.detach(), 'point_pos_num': pos_normalizer.detach()})
        return point_loss_cls, tb_dict

    def get_box_layer_loss(self, tb_dict=None):
        """:172-191, the terms added in float64 and rounded once, as get_cls_layer_loss."""
        if self.reg_loss_func is None:
            raise NotImplementedError("LOSS_REG %r (WeightedSmoothL1Loss)" % (self.model_cfg['LOSS_CONFIG'].get('LOSS_REG', None),))
        pos_mask = self.forward_ret_dict['point_cls_labels'] > 0
        point_box_labels = self.forward_ret_dict['point_box_labels']
        point_box_preds = self.forward_ret_dict['point_box_preds']

        reg_weights = pos_mask.float()
        pos_normalizer = pos_mask.sum().float()
        reg_weights = reg_weights / torch.clamp(pos_normalizer, min=1.0)

        point_loss_box_src = self.reg_loss_func(point_box_preds[None, ...], point_box_labels[None, ...], weights=reg_weights[None, ...])
        point_loss_box = point_loss_box_src.sum(dtype=torch.float64).to(point_loss_box_src.dtype)

        point_loss_box = point_loss_box * self.model_cfg['LOSS_CONFIG']['LOSS_WEIGHTS']['point_box_weight']
        if tb_dict is None:
            tb_dict = {}
        tb_dict.update({'point_loss_box': point_loss_box.detach()})
        return point_loss_box, tb_dict

    def generate_predicted_boxes(self, points, point_cls_preds, point_box_preds):
        """:193-207: points (N, 3), point_cls_preds (N, num_class), point_box_preds (N, code_size) -> the class scores and the
        boxes decoded against the points with the mean size of the best class."""
        _, pred_classes = point_cls_preds.max(dim=-1)
        point_box_preds = self.box_coder.decode_torch(point_box_preds, points, pred_classes + 1)
        return point_cls_preds, point_box_preds

    def forward(self, **kwargs):
        raise NotImplementedError


class PointHeadSimple(PointHeadTemplate):
    def __init__(self, num_class, input_channels, model_cfg, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        self.cls_layers = self.make_fc_layers(fc_cfg=model_cfg['CLS_FC'], input_channels=input_channels, output_channels=num_class)

    def assign_targets(self, input_dict):
        """point_coords (B * N, 4) [bs_idx, x, y, z], gt_boxes (B, M, 8) -> {'point_cls_labels': (B * N) int64, ...}"""
        point_coords = input_dict['point_coords']
        gt_boxes = input_dict['gt_boxes']
        assert gt_boxes.dim() == 3, 'gt_boxes.shape=%s' % str(gt_boxes.shape)
        assert point_coords.dim() == 2, 'points.shape=%s' % str(point_coords.shape)
        return self.assign_stack_targets(points=point_coords, gt_boxes=gt_boxes, set_ignore_flag=True, use_ball_constraint=False,
                                         ret_part_labels=False, extra_width=self.model_cfg['TARGET_CONFIG']['GT_EXTRA_WIDTH'])

    def get_loss(self, tb_dict=None):
        tb_dict = {} if tb_dict is None else tb_dict
        point_loss_cls, tb_dict_1 = self.get_cls_layer_loss()
        tb_dict.update(tb_dict_1)
        return point_loss_cls, tb_dict

    def forward(self, batch_dict):
        """point_features (or point_features_before_fusion) (B * N, C), point_coords -> point_cls_scores (B * N)."""
        if self.model_cfg.get('USE_POINT_FEATURES_BEFORE_FUSION', False):
            point_features = batch_dict['point_features_before_fusion']
        else:
            point_features = batch_dict['point_features']
        point_cls_preds = self.cls_layers(point_features)                       # (total_points, num_class)
        ret_dict = {'point_cls_preds': point_cls_preds}
        point_cls_scores = torch.sigmoid(point_cls_preds)
        batch_dict['point_cls_scores'], _ = point_cls_scores.max(dim=-1)
        if self.training:
            ret_dict['point_cls_labels'] = self.assign_targets(batch_dict)['point_cls_labels']
        self.forward_ret_dict = ret_dict
        return batch_dict


class PointHeadBox(PointHeadTemplate):
    """The point head of PointRCNN (point_head_box.py): a score and a box from every point."""

    def __init__(self, num_class, input_channels, model_cfg, predict_boxes_when_training=False, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        self.predict_boxes_when_training = predict_boxes_when_training
        self.cls_layers = self.make_fc_layers(fc_cfg=model_cfg['CLS_FC'], input_channels=input_channels, output_channels=num_class)
        target_cfg = model_cfg['TARGET_CONFIG']
        self.box_coder = getattr(box_coder_utils, target_cfg['BOX_CODER'])(**target_cfg['BOX_CODER_CONFIG'])
        self.box_layers = self.make_fc_layers(fc_cfg=model_cfg['REG_FC'], input_channels=input_channels,
                                              output_channels=self.box_coder.code_size)

    def assign_targets(self, input_dict):
        """point_coords (B * N, 4) [bs_idx, x, y, z], gt_boxes (B, M, 8) -> point_cls_labels (B * N) int64 and point_box_labels
        (B * N, code_size)."""
        point_coords = input_dict['point_coords']
        gt_boxes = input_dict['gt_boxes']
        assert gt_boxes.dim() == 3, 'gt_boxes.shape=%s' % str(gt_boxes.shape)
        assert point_coords.dim() == 2, 'points.shape=%s' % str(point_coords.shape)
        return self.assign_stack_targets(points=point_coords, gt_boxes=gt_boxes, set_ignore_flag=True, use_ball_constraint=False,
                                         ret_part_labels=False, ret_box_labels=True,
                                         extra_width=self.model_cfg['TARGET_CONFIG']['GT_EXTRA_WIDTH'])

    def get_loss(self, tb_dict=None):
        tb_dict = {} if tb_dict is None else tb_dict
        point_loss_cls, tb_dict_1 = self.get_cls_layer_loss()
        point_loss_box, tb_dict_2 = self.get_box_layer_loss()
        tb_dict.update(tb_dict_1)
        tb_dict.update(tb_dict_2)
        return point_loss_cls + point_loss_box, tb_dict

    def forward(self, batch_dict):
        """point_features (B * N, C), point_coords (B * N, 4) -> point_cls_scores (B * N); in eval, or in training under a RoI
        head, also batch_cls_preds (B * N, num_class), batch_box_preds (B * N, 7) and batch_index."""
        if self.model_cfg.get('USE_POINT_FEATURES_BEFORE_FUSION', False):
            point_features = batch_dict['point_features_before_fusion']
        else:
            point_features = batch_dict['point_features']
        point_cls_preds = self.cls_layers(point_features)                       # (total_points, num_class)
        point_box_preds = self.box_layers(point_features)                       # (total_points, box_code_size)
        point_cls_preds_max, _ = point_cls_preds.max(dim=-1)
        batch_dict['point_cls_scores'] = torch.sigmoid(point_cls_preds_max)

        ret_dict = {'point_cls_preds': point_cls_preds, 'point_box_preds': point_box_preds}
        if self.training:
            targets_dict = self.assign_targets(batch_dict)
            ret_dict['point_cls_labels'] = targets_dict['point_cls_labels']
            ret_dict['point_box_labels'] = targets_dict['point_box_labels']
        if not self.training or self.predict_boxes_when_training:
            point_cls_preds, point_box_preds = self.generate_predicted_boxes(
                points=batch_dict['point_coords'][:, 1:4], point_cls_preds=point_cls_preds, point_box_preds=point_box_preds)
            batch_dict['batch_cls_preds'] = point_cls_preds
            batch_dict['batch_box_preds'] = point_box_preds
            batch_dict['batch_index'] = batch_dict['point_coords'][:, 0]
            batch_dict['cls_preds_normalized'] = False
        self.forward_ret_dict = ret_dict
        return batch_dict
