"""RoIHeadTemplate (pcdet/models/roi_heads/roi_head_template.py): what every two-stage head of the reference shares --
`proposal_layer` (first-stage predictions -> rois / roi_scores / roi_labels through per-scene NMS), `assign_targets`
(ProposalTargetLayer and the canonical transformation), the fc stacks, the box decoding and the rcnn losses -- for the
whole batch at once and without a host read anywhere on the training path.  It also holds, once, what the reference's heads
each repeat: the two ends of forward() (`proposals_and_targets`, `keep_predictions`), the RoI grid points, the Conv1d shared
stack and `init_weights`.

Where the reference loops over scenes (proposal_layer) this uses model_nms_utils.class_agnostic_nms_batched; where it
loops over scenes and classes and draws on the host (assign_targets) this uses proposal_target_layer (csrc/roi_targets.hip),
which also applies the canonical transformation, so assign_targets adds nothing after it.  The losses are plain torch, the
reference's arithmetic, with its `.item()` reads replaced: tb_dict values are 0-dim device tensors, the foreground count
stays on the device, and the foreground subset of the corner loss is taken by masking (a scene batch without foreground
then reports rcnn_loss_corner = 0 where the reference leaves the key out).

Out of scope: MULTI_CLASSES_NMS (NotImplementedError, as in the reference), boxes with velocities."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import box_coder_utils, box_utils, loss_utils
from .model_nms_utils import class_agnostic_nms_batched
from .proposal_target_layer import ProposalTargetLayer


class RoIHeadTemplate(nn.Module):
    def __init__(self, num_class, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        target_cfg = model_cfg['TARGET_CONFIG']
        self.box_coder = getattr(box_coder_utils, target_cfg['BOX_CODER'])(**target_cfg.get('BOX_CODER_CONFIG', {}))
        self.proposal_target_layer = ProposalTargetLayer(roi_sampler_cfg=target_cfg)
        self.build_losses(model_cfg['LOSS_CONFIG'])
        self.forward_ret_dict = None

    def build_losses(self, losses_cfg):
        self.add_module('reg_loss_func',
                        loss_utils.WeightedSmoothL1Loss(code_weights=losses_cfg['LOSS_WEIGHTS']['code_weights']))

    def make_fc_layers(self, input_channels, output_channels, fc_list):
        """:29-43, the same module order and so the same state-dict keys."""
        fc_layers = []
        pre_channel = input_channels
        for k in range(len(fc_list)):
            fc_layers.extend([nn.Conv1d(pre_channel, fc_list[k], kernel_size=1, bias=False), nn.BatchNorm1d(fc_list[k]),
                              nn.ReLU()])
            pre_channel = fc_list[k]
            if self.model_cfg['DP_RATIO'] >= 0 and k == 0:
                fc_layers.append(nn.Dropout(self.model_cfg['DP_RATIO']))
        fc_layers.append(nn.Conv1d(pre_channel, output_channels, kernel_size=1, bias=True))
        return nn.Sequential(*fc_layers)

    def make_shared_fc_layers(self, input_channels, fc_list):
        """The Conv1d-BN-ReLU stack in front of the prediction stacks (pvrcnn_head.py:33-43, second_head.py:33-43), a Dropout
        between its blocks.  Returns the stack and its output width."""
        fc_layers = []
        pre_channel = input_channels
        for k in range(len(fc_list)):
            fc_layers.extend([nn.Conv1d(pre_channel, fc_list[k], kernel_size=1, bias=False), nn.BatchNorm1d(fc_list[k]),
                              nn.ReLU()])
            pre_channel = fc_list[k]
            if k != len(fc_list) - 1 and self.model_cfg['DP_RATIO'] > 0:
                fc_layers.append(nn.Dropout(self.model_cfg['DP_RATIO']))
        return nn.Sequential(*fc_layers), pre_channel

    def init_weights(self, weight_init='xavier'):
        """pvrcnn_head.py:48-65 / pointrcnn_head.py:74-91: every Conv of the head, then reg_layers' last one again."""
        if weight_init == 'kaiming':
            init_func = nn.init.kaiming_normal_
        elif weight_init == 'xavier':
            init_func = nn.init.xavier_normal_
        elif weight_init == 'normal':
            init_func = nn.init.normal_
        else:
            raise NotImplementedError
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                if weight_init == 'normal':
                    init_func(m.weight, mean=0, std=0.001)
                else:
                    init_func(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)

    @torch.no_grad()
    def proposal_layer(self, batch_dict, nms_config):
        """:45-102 for the whole batch.  batch_cls_preds (B, N, num_class | 1) with batch_box_preds (B, N, 7), or both with
        the rows of all scenes stacked and `batch_index` given (equal rows per scene, the assumption post_processing
        makes).  The raw max over the classes is the score, there is no score threshold, and the survivors of the
        class-agnostic NMS fill rois (B, NMS_POST_MAXSIZE, 7), roi_scores and roi_labels = label + 1 from the left;
        the zero padding therefore carries label 1, as in the reference."""
        if batch_dict.get('rois', None) is not None:
            return batch_dict
        B = batch_dict['batch_size']
        box_preds, cls_preds = batch_dict['batch_box_preds'], batch_dict['batch_cls_preds']
        if batch_dict.get('batch_index', None) is not None:
            assert cls_preds.dim() == 2
            box_preds = box_preds.view(B, -1, box_preds.shape[-1])
            cls_preds = cls_preds.view(B, box_preds.shape[1], -1)
        else:
            assert cls_preds.dim() == 3
        if box_preds.shape[-1] > 7:
            raise NotImplementedError("boxes with velocities are not supported")
        if nms_config['MULTI_CLASSES_NMS']:
            raise NotImplementedError
        post = int(nms_config['NMS_POST_MAXSIZE'])
        scores, labels = torch.max(cls_preds, dim=-1)
        selected, sel_scores, _ = class_agnostic_nms_batched(scores, box_preds, nms_config)
        K = selected.shape[1]
        ok = selected >= 0
        safe = selected.clamp(min=0)
        rois = box_preds.new_zeros((B, post, box_preds.shape[-1]))
        roi_scores = box_preds.new_zeros((B, post))
        roi_labels = torch.zeros((B, post), dtype=torch.long, device=box_preds.device)
        picked = torch.gather(box_preds, 1, safe.unsqueeze(-1).expand(-1, -1, box_preds.shape[-1]))
        rois[:, :K] = torch.where(ok.unsqueeze(-1), picked, torch.zeros_like(picked))
        roi_scores[:, :K] = sel_scores
        roi_labels[:, :K] = torch.where(ok, torch.gather(labels, 1, safe), torch.zeros_like(safe))
        batch_dict['rois'] = rois
        batch_dict['roi_scores'] = roi_scores
        batch_dict['roi_labels'] = roi_labels + 1
        batch_dict['has_class_labels'] = True if cls_preds.shape[-1] > 1 else False
        batch_dict.pop('batch_index', None)
        return batch_dict

    def assign_targets(self, batch_dict, seed=None, draws=None, check=False):
        """:104-134: the targets dict with gt_of_rois in each RoI's canonical frame and gt_of_rois_src the sampled GT rows.
        seed / draws / check: see ProposalTargetLayer.forward."""
        return self.proposal_target_layer.forward(batch_dict, seed=seed, draws=draws, check=check)

    def proposals_and_targets(self, batch_dict):
        """What every head's forward() opens with: the proposals of the current mode and, in training, the sampled targets
        (batch_dict's 'roi_target_seed' / 'roi_target_draws' are ProposalTargetLayer.forward's seed / draws), whose rois and
        roi_labels replace the proposals in the batch.  Returns the targets dict (the batch itself in eval)."""
        targets_dict = self.proposal_layer(batch_dict, nms_config=self.model_cfg['NMS_CONFIG']['TRAIN' if self.training else 'TEST'])
        if self.training:
            targets_dict = self.assign_targets(batch_dict, seed=batch_dict.get('roi_target_seed'),
                                               draws=batch_dict.get('roi_target_draws'))
            batch_dict['rois'] = targets_dict['rois']
            batch_dict['roi_labels'] = targets_dict['roi_labels']
        return targets_dict

    def keep_predictions(self, batch_dict, targets_dict, rcnn_cls, rcnn_reg):
        """What a head with a class and a box branch closes forward() with: the decoded boxes into the batch in eval, the raw
        predictions next to their targets into forward_ret_dict in training."""
        if not self.training:
            batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(
                batch_size=batch_dict['batch_size'], rois=batch_dict['rois'], cls_preds=rcnn_cls, box_preds=rcnn_reg)
            batch_dict['batch_cls_preds'] = batch_cls_preds
            batch_dict['batch_box_preds'] = batch_box_preds
            batch_dict['cls_preds_normalized'] = False
        else:
            targets_dict['rcnn_cls'] = rcnn_cls
            targets_dict['rcnn_reg'] = rcnn_reg
            self.forward_ret_dict = targets_dict
        return batch_dict

    def get_global_grid_points_of_roi(self, rois, grid_size):
        """voxelrcnn_head.py / pvrcnn_head.py: rois (..., 7 + C) -> the GRID_SIZE^3 grid points of each RoI in the lidar frame
        and in the RoI's own, (BxN, 6x6x6, 3) each."""
        rois = rois.view(-1, rois.shape[-1])
        batch_size_rcnn = rois.shape[0]
        local_roi_grid_points = self.get_dense_grid_points(rois, batch_size_rcnn, grid_size)    # (B, 6x6x6, 3)
        global_roi_grid_points = box_utils.rotate_points_along_z(local_roi_grid_points.clone(), rois[:, 6]).squeeze(dim=1)
        global_center = rois[:, 0:3].clone()
        global_roi_grid_points += global_center.unsqueeze(dim=1)
        return global_roi_grid_points, local_roi_grid_points

    @staticmethod
    def get_dense_grid_points(rois, batch_size_rcnn, grid_size):
        """The reference's `faked_features.nonzero()` of an all-ones cube is the index grid in row-major order; built here
        without the host read nonzero() makes."""
        axis = torch.arange(grid_size, device=rois.device)
        dense_idx = torch.stack(torch.meshgrid(axis, axis, axis, indexing='ij'), dim=-1).view(-1, 3)
        dense_idx = dense_idx.repeat(batch_size_rcnn, 1, 1).to(rois.dtype)                       # (B, 6x6x6, 3)
        local_roi_size = rois.view(batch_size_rcnn, -1)[:, 3:6]
        roi_grid_points = (dense_idx + 0.5) / grid_size * local_roi_size.unsqueeze(dim=1) \
            - (local_roi_size.unsqueeze(dim=1) / 2)
        return roi_grid_points

    def get_box_reg_layer_loss(self, forward_ret_dict):
        loss_cfgs = self.model_cfg['LOSS_CONFIG']
        code_size = self.box_coder.code_size
        reg_valid_mask = forward_ret_dict['reg_valid_mask'].view(-1)
        gt_boxes3d_ct = forward_ret_dict['gt_of_rois'][..., 0:code_size]
        gt_of_rois_src = forward_ret_dict['gt_of_rois_src'][..., 0:code_size].view(-1, code_size)
        rcnn_reg = forward_ret_dict['rcnn_reg']                    # (rcnn_batch_size, C)
        roi_boxes3d = forward_ret_dict['rois']
        rcnn_batch_size = gt_boxes3d_ct.view(-1, code_size).shape[0]

        fg_mask = reg_valid_mask > 0
        fg_count = fg_mask.sum().clamp(min=1).float()              # max(fg_sum, 1), on the device
        tb_dict = {}
        if loss_cfgs['REG_LOSS'] != 'smooth-l1':
            raise NotImplementedError

        rois_anchor = roi_boxes3d.clone().detach().view(-1, code_size)
        rois_anchor[:, 0:3] = 0
        rois_anchor[:, 6] = 0
        reg_targets = self.box_coder.encode_torch(gt_boxes3d_ct.view(rcnn_batch_size, code_size), rois_anchor)
        rcnn_loss_reg = self.reg_loss_func(rcnn_reg.view(rcnn_batch_size, -1).unsqueeze(dim=0), reg_targets.unsqueeze(dim=0))
        rcnn_loss_reg = (rcnn_loss_reg.view(rcnn_batch_size, -1) * fg_mask.unsqueeze(dim=-1).float()).sum() / fg_count
        rcnn_loss_reg = rcnn_loss_reg * loss_cfgs['LOSS_WEIGHTS']['rcnn_reg_weight']
        tb_dict['rcnn_loss_reg'] = rcnn_loss_reg.detach()

        if loss_cfgs['CORNER_LOSS_REGULARIZATION']:
            # every row is decoded, background rows from zero codes so that nothing of them (an overflowing exp) reaches the
            # sum or the gradient; the mean over the foreground rows is a masked sum over the count
            fg_col = fg_mask.unsqueeze(dim=-1)
            codes = torch.where(fg_col, rcnn_reg.view(rcnn_batch_size, -1), torch.zeros_like(rcnn_reg.view(rcnn_batch_size, -1)))
            rois_flat = roi_boxes3d.view(-1, code_size)
            batch_anchors = rois_flat.clone().detach()
            batch_anchors[:, 0:3] = 0
            rcnn_boxes3d = self.box_coder.decode_torch(codes, batch_anchors)
            rcnn_boxes3d = box_utils.rotate_points_along_z(rcnn_boxes3d.unsqueeze(dim=1), rois_flat[:, 6]).squeeze(dim=1)
            rcnn_boxes3d = torch.cat([rcnn_boxes3d[:, 0:3] + rois_flat[:, 0:3], rcnn_boxes3d[:, 3:]], dim=-1)
            loss_corner = loss_utils.get_corner_loss_lidar(rcnn_boxes3d[:, 0:7], gt_of_rois_src[:, 0:7])
            loss_corner = torch.where(fg_mask, loss_corner, torch.zeros_like(loss_corner)).sum() / fg_count
            loss_corner = loss_corner * loss_cfgs['LOSS_WEIGHTS']['rcnn_corner_weight']
            rcnn_loss_reg = rcnn_loss_reg + loss_corner
            tb_dict['rcnn_loss_corner'] = loss_corner.detach()
        return rcnn_loss_reg, tb_dict

    def get_box_cls_layer_loss(self, forward_ret_dict):
        loss_cfgs = self.model_cfg['LOSS_CONFIG']
        rcnn_cls = forward_ret_dict['rcnn_cls']
        rcnn_cls_labels = forward_ret_dict['rcnn_cls_labels'].view(-1)
        if loss_cfgs['CLS_LOSS'] == 'BinaryCrossEntropy':
            # the -1 of 'cls' targets is masked below; clamped here because binary_cross_entropy checks its target range
            batch_loss_cls = F.binary_cross_entropy(torch.sigmoid(rcnn_cls.view(-1)), rcnn_cls_labels.float().clamp(min=0),
                                                    reduction='none')
        elif loss_cfgs['CLS_LOSS'] == 'CrossEntropy':
            batch_loss_cls = F.cross_entropy(rcnn_cls, rcnn_cls_labels, reduction='none', ignore_index=-1)
        else:
            raise NotImplementedError
        cls_valid_mask = (rcnn_cls_labels >= 0).float()
        rcnn_loss_cls = (batch_loss_cls * cls_valid_mask).sum() / torch.clamp(cls_valid_mask.sum(), min=1.0)
        rcnn_loss_cls = rcnn_loss_cls * loss_cfgs['LOSS_WEIGHTS']['rcnn_cls_weight']
        return rcnn_loss_cls, {'rcnn_loss_cls': rcnn_loss_cls.detach()}

    def get_loss(self, tb_dict=None):
        tb_dict = {} if tb_dict is None else tb_dict
        rcnn_loss_cls, cls_tb_dict = self.get_box_cls_layer_loss(self.forward_ret_dict)
        tb_dict.update(cls_tb_dict)
        rcnn_loss_reg, reg_tb_dict = self.get_box_reg_layer_loss(self.forward_ret_dict)
        tb_dict.update(reg_tb_dict)
        rcnn_loss = rcnn_loss_cls + rcnn_loss_reg
        tb_dict['rcnn_loss'] = rcnn_loss.detach()
        return rcnn_loss, tb_dict

    def generate_predicted_boxes(self, batch_size, rois, cls_preds, box_preds):
        """:233-261: rois (B, N, 7), cls_preds (BN, num_class), box_preds (BN, code_size) -> batch_cls_preds (B, N, ·) and the
        decoded boxes (B, N, code_size) in the lidar frame."""
        code_size = self.box_coder.code_size
        batch_cls_preds = cls_preds.view(batch_size, -1, cls_preds.shape[-1])
        batch_box_preds = box_preds.view(batch_size, -1, code_size)
        roi_ry = rois[:, :, 6].reshape(-1)
        roi_xyz = rois[:, :, 0:3].reshape(-1, 3)
        local_rois = rois.clone().detach()
        local_rois[:, :, 0:3] = 0
        batch_box_preds = self.box_coder.decode_torch(batch_box_preds, local_rois).view(-1, code_size)
        batch_box_preds = box_utils.rotate_points_along_z(batch_box_preds.unsqueeze(dim=1), roi_ry).squeeze(dim=1)
        batch_box_preds = torch.cat([batch_box_preds[:, 0:3] + roi_xyz, batch_box_preds[:, 3:]], dim=-1)
        return batch_cls_preds, batch_box_preds.view(batch_size, -1, code_size)
