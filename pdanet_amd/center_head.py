"""CenterHead and SeparateHead (pcdet/models/dense_heads/center_head.py) with the reference's constructor signatures,
config keys and state-dict keys (shared_conv.*, heads_list.{i}.{name}.*), so a reference checkpoint loads with
strict=True.  The convolutions stay in torch; target assignment, both losses and the box decoding are the operators of
centernet_utils.py (csrc/center_head.hip) and read nothing back to the host: assign_targets + get_loss + backward replay
from one captured graph.

Departures from the reference:
- gt_boxes is not written.  The reference writes the head-local class index back into the caller's tensor
  (`temp_box[-1] = ...` on a view), so later heads see re-labelled boxes whenever CLASS_NAMES_EACH_HEAD is not in class
  order; here every head selects by the original labels.
- tb_dict holds 0-dim device tensors, not .item() floats.
- generate_predicted_boxes returns the padded form of model_nms_utils.post_processing (pred_boxes, pred_scores,
  pred_labels with 0 = padding, num_pred), which to_pred_dicts, recall_record, RecallRecorder and the evaluators take.
- ties among heat-map scores are left to torch.topk by the reference and are outside the parity claim; circle_nms raises
  NotImplementedError (the reference asserts False there)."""
import copy

import torch
import torch.nn as nn
from torch.nn.init import kaiming_normal_

from . import centernet_utils
from .model_nms_utils import class_agnostic_nms_batched


class SeparateHead(nn.Module):
    def __init__(self, input_channels, sep_head_dict, init_bias=-2.19, use_bias=False):
        super().__init__()
        self.sep_head_dict = sep_head_dict
        for name, spec in sep_head_dict.items():
            layers = [nn.Sequential(nn.Conv2d(input_channels, input_channels, kernel_size=3, stride=1, padding=1, bias=use_bias),
                                    nn.BatchNorm2d(input_channels), nn.ReLU())
                      for _ in range(spec['num_conv'] - 1)]
            layers.append(nn.Conv2d(input_channels, spec['out_channels'], kernel_size=3, stride=1, padding=1, bias=True))
            branch = nn.Sequential(*layers)
            if 'hm' in name:
                branch[-1].bias.data.fill_(init_bias)
            else:
                for m in branch.modules():
                    if isinstance(m, nn.Conv2d):
                        kaiming_normal_(m.weight.data)
                        if m.bias is not None:
                            nn.init.constant_(m.bias, 0)
            setattr(self, name, branch)

    def forward(self, x):
        return {name: getattr(self, name)(x) for name in self.sep_head_dict}


class CenterHead(nn.Module):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, voxel_size,
                 predict_boxes_when_training=True):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.grid_size = grid_size
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.voxel_size = [float(v) for v in voxel_size]
        self.feature_map_stride = model_cfg['TARGET_ASSIGNER_CONFIG'].get('FEATURE_MAP_STRIDE', None)
        self.class_names = list(class_names)
        self.class_names_each_head = [[x for x in names if x in self.class_names] for names in model_cfg['CLASS_NAMES_EACH_HEAD']]
        # host lists where the reference keeps device tensors: the decode kernel takes the mapping as an argument
        self.class_id_mapping_each_head = [[self.class_names.index(x) for x in names] for names in self.class_names_each_head]
        total = sum(len(x) for x in self.class_names_each_head)
        assert total == len(self.class_names), 'class_names_each_head=%s' % (self.class_names_each_head,)
        self.layout = centernet_utils.HeadLayout(self.class_names, self.class_names_each_head)

        use_bias = model_cfg.get('USE_BIAS_BEFORE_NORM', False)
        shared = model_cfg['SHARED_CONV_CHANNEL']
        self.shared_conv = nn.Sequential(nn.Conv2d(input_channels, shared, 3, stride=1, padding=1, bias=use_bias),
                                         nn.BatchNorm2d(shared), nn.ReLU())
        self.heads_list = nn.ModuleList()
        self.separate_head_cfg = model_cfg['SEPARATE_HEAD_CFG']
        for names in self.class_names_each_head:
            head_dict = copy.deepcopy(self.separate_head_cfg['HEAD_DICT'])
            head_dict['hm'] = dict(out_channels=len(names), num_conv=model_cfg['NUM_HM_CONV'])
            self.heads_list.append(SeparateHead(input_channels=shared, sep_head_dict=head_dict, init_bias=-2.19, use_bias=use_bias))
        self.predict_boxes_when_training = predict_boxes_when_training
        self.forward_ret_dict = {}

    def assign_targets(self, gt_boxes, feature_map_size=None, **kwargs):
        """gt_boxes (B, M, 8 or 10) on the device, feature_map_size (H, W) -> the reference's ret_dict (lists per head of
        heatmaps, target_boxes, inds, masks).  One launch for the batch and all heads; nothing is read back and gt_boxes
        is not written."""
        cfg = self.model_cfg['TARGET_ASSIGNER_CONFIG']
        with torch.no_grad():
            return centernet_utils.center_targets(
                gt_boxes.contiguous(), self.layout, feature_map_size, self.point_cloud_range, self.voxel_size,
                cfg['FEATURE_MAP_STRIDE'], cfg['NUM_MAX_OBJS'], cfg['GAUSSIAN_OVERLAP'], cfg['MIN_RADIUS'])

    def get_loss(self):
        """(loss, tb_dict): per head the focal loss on the heat-map logits times cls_weight and the L1 loss over
        HEAD_ORDER times code_weights and loc_weight; tb_dict values are 0-dim device tensors."""
        pred_dicts = self.forward_ret_dict['pred_dicts']
        target_dicts = self.forward_ret_dict['target_dicts']
        weights = self.model_cfg['LOSS_CONFIG']['LOSS_WEIGHTS']
        tb_dict = {}
        loss = 0
        for idx, pred_dict in enumerate(pred_dicts):
            hm_loss = centernet_utils.focal_loss(pred_dict['hm'], target_dicts['heatmaps'][idx], weights['cls_weight'])
            maps = [pred_dict[name] for name in self.separate_head_cfg['HEAD_ORDER']]
            loc_loss, _ = centernet_utils.reg_loss(maps, target_dicts['masks'][idx], target_dicts['inds'][idx],
                                                   target_dicts['target_boxes'][idx], weights['code_weights'],
                                                   weights['loc_weight'])
            loss = loss + hm_loss + loc_loss
            tb_dict['hm_loss_head_%d' % idx] = hm_loss.detach()
            tb_dict['loc_loss_head_%d' % idx] = loc_loss.detach()
        tb_dict['rpn_loss'] = loss.detach()
        return loss, tb_dict

    @torch.no_grad()
    def generate_predicted_boxes(self, batch_size, pred_dicts):
        """The heads' decoded boxes after the per-head class-agnostic NMS, concatenated per scene in head order, in the
        padded form of model_nms_utils.post_processing: pred_boxes (B, P, 7 or 9), pred_scores (B, P), pred_labels (B, P)
        int64 (label + 1, 0 = padding), num_pred (B) int32; P = the heads' NMS_POST_MAXSIZE (or MAX_OBJ_PER_SAMPLE) summed.
        No host read."""
        cfg = self.model_cfg['POST_PROCESSING']
        nms_cfg = cfg['NMS_CONFIG']
        if nms_cfg['NMS_TYPE'] == 'circle_nms':
            raise NotImplementedError("circle_nms (the reference asserts False on this path)")
        per_head = []
        for idx, pred_dict in enumerate(pred_dicts):
            boxes, scores, labels = centernet_utils.decode_topk(
                pred_dict if 'vel' in self.separate_head_cfg['HEAD_ORDER'] else {k: v for k, v in pred_dict.items() if k != 'vel'},
                cfg['MAX_OBJ_PER_SAMPLE'], self.class_id_mapping_each_head[idx], self.point_cloud_range, self.voxel_size,
                self.feature_map_stride, cfg['POST_CENTER_LIMIT_RANGE'], cfg['SCORE_THRESH'])
            selected, sel_scores, num = class_agnostic_nms_batched(scores, boxes, nms_cfg, valid=scores > float('-inf'))
            ok = selected >= 0
            safe = selected.clamp(min=0)
            sel_boxes = torch.gather(boxes, 1, safe.unsqueeze(-1).expand(-1, -1, boxes.shape[-1])) * ok.unsqueeze(-1)
            sel_labels = torch.where(ok, torch.gather(labels, 1, safe) + 1, torch.zeros_like(safe))
            per_head.append((sel_boxes, sel_scores, sel_labels, num))
        if len(per_head) == 1:
            b, s, l, n = per_head[0]
            return {'pred_boxes': b, 'pred_scores': s, 'pred_labels': l, 'num_pred': n}
        P = sum(h[0].shape[1] for h in per_head)
        dev, cols = per_head[0][0].device, per_head[0][0].shape[-1]
        out_b = torch.zeros((batch_size, P + 1, cols), dtype=torch.float32, device=dev)      # column P collects the padding
        out_s = torch.zeros((batch_size, P + 1), dtype=torch.float32, device=dev)
        out_l = torch.zeros((batch_size, P + 1), dtype=torch.int64, device=dev)
        offset = torch.zeros((batch_size,), dtype=torch.int64, device=dev)
        for b, s, l, n in per_head:
            k = b.shape[1]
            slot = torch.arange(k, device=dev).unsqueeze(0)
            dest = torch.where(slot < n.unsqueeze(1), offset.unsqueeze(1) + slot, torch.full_like(slot, P))
            out_b.scatter_(1, dest.unsqueeze(-1).expand(-1, -1, cols), b)
            out_s.scatter_(1, dest, s)
            out_l.scatter_(1, dest, l)
            offset = offset + n.to(torch.int64)
        return {'pred_boxes': out_b[:, :P].contiguous(), 'pred_scores': out_s[:, :P].contiguous(),
                'pred_labels': out_l[:, :P].contiguous(), 'num_pred': offset.to(torch.int32)}

    @staticmethod
    def reorder_rois_for_refining(batch_size, padded):
        """rois (B, P, 7 or 9), roi_scores (B, P), roi_labels (B, P) int64 from generate_predicted_boxes' padded tensors:
        they are zero beyond each scene's count already, so nothing is read (the reference sizes them to the longest
        scene, at least 1)."""
        return padded['pred_boxes'], padded['pred_scores'], padded['pred_labels']

    def forward(self, data_dict):
        spatial_features_2d = data_dict['spatial_features_2d']
        x = self.shared_conv(spatial_features_2d)
        pred_dicts = [head(x) for head in self.heads_list]
        if self.training:
            self.forward_ret_dict['target_dicts'] = self.assign_targets(
                data_dict['gt_boxes'], feature_map_size=spatial_features_2d.size()[2:],
                feature_map_stride=data_dict.get('spatial_features_2d_strides', None))
        self.forward_ret_dict['pred_dicts'] = pred_dicts
        if not self.training or self.predict_boxes_when_training:
            padded = self.generate_predicted_boxes(data_dict['batch_size'], pred_dicts)
            if self.predict_boxes_when_training:
                rois, roi_scores, roi_labels = self.reorder_rois_for_refining(data_dict['batch_size'], padded)
                data_dict['rois'] = rois
                data_dict['roi_scores'] = roi_scores
                data_dict['roi_labels'] = roi_labels
                data_dict['has_class_labels'] = True
            else:
                data_dict['final_padded'] = padded
        return data_dict
