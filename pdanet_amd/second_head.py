"""SECONDHead (pcdet/models/roi_heads/second_head.py) for kitti_models/second_iou.yaml: rotated RoI-grid pooling over the
2D backbone's BEV map, a shared fc stack and an IoU branch, under the reference's module names (shared_fc_layer, iou_layers),
so a reference checkpoint loads with strict=True.

roi_grid_pool: the reference loops over the scenes on the host, builds an (R, G, G, 2) grid with affine_grid and samples an
`expand`ed (R, C, H, W) view of the scene's map with grid_sample, with cuDNN switched off around the loop.  Here
`bev_roi_grid_pool` (csrc/bev_roi_pool.hip) does the whole batch in one launch; its arithmetic is what torch computes for the
reference's code (align_corners=False in both calls), stated in include/pda_train.h.  PDA_BEV_ROI_POOL=composed selects the
reference's torch composition instead (the benchmark's baseline, benchmarks/second_iou.py).  The features are detached, as
in the reference: the pooled tensor does not require grad and the first Conv1d needs only its weight gradient.

The geometry (POINT_CLOUD_RANGE, VOXEL_SIZE) comes from the constructor, not from batch_dict['dataset_cfg'].  The loss is
plain torch, the reference's arithmetic with its `.item()` reads replaced: tb_dict values are 0-dim device tensors, and the
training path reads nothing on the host.

Target sampling: batch_dict may carry 'roi_target_seed' or 'roi_target_draws' (ProposalTargetLayer.forward's seed / draws).

Out of scope: boxes with velocities, IOU_LOSS 'focalbce' (the reference calls loss_utils.sigmoid_focal_cls_loss, which it
does not have), MULTI_CLASSES_NMS."""
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import loss_utils
from .config import fused_or_composed
from .pointnet2_batch_cuda import F32, _call, _chk
from .roi_head_template import RoIHeadTemplate

# 'fused' (default) or 'composed', read when the head pools
ENV = "PDA_BEV_ROI_POOL"
pool_path = partial(fused_or_composed, ENV)
IOU_LOSSES = ('BinaryCrossEntropy', 'L2', 'smoothL1')


def bev_roi_grid_pool(bev, rois, grid_size, min_x, min_y, cell_x, cell_y):
    """bev (B, C, H, W) float32, rois (B, R, 7) float32 [x, y, z, dx, dy, dz, ry] -> (B * R, C, G, G), one launch, no
    gradient.  cell_x / cell_y: the size of a map cell, VOXEL_SIZE * DOWNSAMPLE_RATIO."""
    if bev.dim() != 4 or rois.dim() != 3 or rois.shape[0] != bev.shape[0] or rois.shape[2] != 7:
        raise ValueError("bev must be (B, C, H, W) and rois (B, R, 7), got %s and %s" % (tuple(bev.shape), tuple(rois.shape)))
    bev, rois = bev.detach().contiguous(), rois.detach().contiguous()
    B, C, H, W = (int(v) for v in bev.shape)
    R, G = int(rois.shape[1]), int(grid_size)
    out = torch.empty((B * R, C, G, G), dtype=F32, device=bev.device)
    _call("pda_bev_roi_grid_pool", bev, _chk(bev, "bev", F32), _chk(rois, "rois", F32), _chk(out, "out", F32), B, R, C, H, W, G,
          float(min_x), float(min_y), float(cell_x), float(cell_y))
    return out


def bev_roi_grid_pool_composed(bev, rois, grid_size, min_x, min_y, cell_x, cell_y):
    """The reference's composition (second_head.py:75-108): per scene, theta -> affine_grid -> grid_sample over the expanded
    map, cuDNN off around it.  Works on CPU tensors too."""
    bev, rois = bev.detach(), rois.detach()
    height, width = bev.size(2), bev.size(3)
    pooled = []
    with torch.backends.cudnn.flags(enabled=False):
        for b_id in range(bev.size(0)):
            x1 = (rois[b_id, :, 0] - rois[b_id, :, 3] / 2 - min_x) / cell_x
            x2 = (rois[b_id, :, 0] + rois[b_id, :, 3] / 2 - min_x) / cell_x
            y1 = (rois[b_id, :, 1] - rois[b_id, :, 4] / 2 - min_y) / cell_y
            y2 = (rois[b_id, :, 1] + rois[b_id, :, 4] / 2 - min_y) / cell_y
            cosa, sina = torch.cos(rois[b_id, :, 6]), torch.sin(rois[b_id, :, 6])
            theta = torch.stack((
                (x2 - x1) / (width - 1) * cosa, (x2 - x1) / (width - 1) * (-sina), (x1 + x2 - width + 1) / (width - 1),
                (y2 - y1) / (height - 1) * sina, (y2 - y1) / (height - 1) * cosa, (y1 + y2 - height + 1) / (height - 1)
            ), dim=1).view(-1, 2, 3).to(bev.dtype)
            grid = F.affine_grid(theta, torch.Size((rois.size(1), bev.size(1), grid_size, grid_size)), align_corners=False)
            pooled.append(F.grid_sample(bev[b_id].unsqueeze(0).expand(rois.size(1), bev.size(1), height, width), grid,
                                        mode='bilinear', padding_mode='zeros', align_corners=False))
    return torch.cat(pooled, dim=0)


class SECONDHead(RoIHeadTemplate):
    def __init__(self, backbone_channels=None, model_cfg=None, point_cloud_range=None, voxel_size=None, num_class=1,
                 input_channels=None, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.pool_cfg = model_cfg['ROI_GRID_POOL']
        iou_loss = model_cfg['LOSS_CONFIG']['IOU_LOSS']
        if iou_loss == 'focalbce':
            raise NotImplementedError("IOU_LOSS 'focalbce': the reference calls loss_utils.sigmoid_focal_cls_loss, which it does not have")
        if iou_loss not in IOU_LOSSES:
            raise NotImplementedError("IOU_LOSS %r (%s)" % (iou_loss, ", ".join(IOU_LOSSES)))
        self.min_x, self.min_y = float(point_cloud_range[0]), float(point_cloud_range[1])
        ratio = self.pool_cfg['DOWNSAMPLE_RATIO']
        self.cell_x, self.cell_y = float(voxel_size[0]) * ratio, float(voxel_size[1]) * ratio

        grid = self.pool_cfg['GRID_SIZE']
        self.shared_fc_layer, pre_channel = self.make_shared_fc_layers(self.pool_cfg['IN_CHANNEL'] * grid * grid, model_cfg['SHARED_FC'])
        self.iou_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=1, fc_list=model_cfg['IOU_FC'])
        self.init_weights()

    def init_weights(self):
        """weight_init='xavier' of the reference, over every Conv1d of the head"""
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.xavier_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def roi_grid_pool(self, batch_dict):
        """rois (B, num_rois, 7), spatial_features_2d (B, C, H, W) -> (B * num_rois, C, GRID_SIZE, GRID_SIZE), detached."""
        rois = batch_dict['rois'].detach()
        if rois.shape[-1] > 7:
            raise NotImplementedError("boxes with velocities are not supported")
        pool = bev_roi_grid_pool if pool_path() == "fused" else bev_roi_grid_pool_composed
        return pool(batch_dict['spatial_features_2d'].detach(), rois, self.pool_cfg['GRID_SIZE'], self.min_x, self.min_y,
                    self.cell_x, self.cell_y)

    def forward(self, batch_dict):
        targets_dict = self.proposals_and_targets(batch_dict)

        pooled_features = self.roi_grid_pool(batch_dict)                                         # (BxN, C, 7, 7)
        batch_size_rcnn = pooled_features.shape[0]
        shared_features = self.shared_fc_layer(pooled_features.view(batch_size_rcnn, -1, 1))
        rcnn_iou = self.iou_layers(shared_features).transpose(1, 2).contiguous().squeeze(dim=1)   # (B*N, 1)

        if not self.training:
            batch_dict['batch_cls_preds'] = rcnn_iou.view(batch_dict['batch_size'], -1, rcnn_iou.shape[-1])
            batch_dict['batch_box_preds'] = batch_dict['rois']
            batch_dict['cls_preds_normalized'] = False
        else:
            targets_dict['rcnn_iou'] = rcnn_iou
            self.forward_ret_dict = targets_dict
        return batch_dict

    def get_loss(self, tb_dict=None):
        tb_dict = {} if tb_dict is None else tb_dict
        rcnn_loss, iou_tb_dict = self.get_box_iou_layer_loss(self.forward_ret_dict)
        tb_dict.update(iou_tb_dict)
        tb_dict['rcnn_loss'] = rcnn_loss.detach()
        return rcnn_loss, tb_dict

    def get_box_iou_layer_loss(self, forward_ret_dict):
        loss_cfgs = self.model_cfg['LOSS_CONFIG']
        rcnn_iou_flat = forward_ret_dict['rcnn_iou'].view(-1)
        rcnn_iou_labels = forward_ret_dict['rcnn_cls_labels'].view(-1)
        if loss_cfgs['IOU_LOSS'] == 'BinaryCrossEntropy':
            batch_loss_iou = F.binary_cross_entropy_with_logits(rcnn_iou_flat, rcnn_iou_labels.to(rcnn_iou_flat.dtype), reduction='none')
        elif loss_cfgs['IOU_LOSS'] == 'L2':
            batch_loss_iou = F.mse_loss(rcnn_iou_flat, rcnn_iou_labels, reduction='none')
        elif loss_cfgs['IOU_LOSS'] == 'smoothL1':
            batch_loss_iou = loss_utils.WeightedSmoothL1Loss.smooth_l1_loss(rcnn_iou_flat - rcnn_iou_labels, 1.0 / 9.0)
        else:
            raise NotImplementedError(loss_cfgs['IOU_LOSS'])
        iou_valid_mask = (rcnn_iou_labels >= 0).float()
        rcnn_loss_iou = (batch_loss_iou * iou_valid_mask).sum() / torch.clamp(iou_valid_mask.sum(), min=1.0)
        rcnn_loss_iou = rcnn_loss_iou * loss_cfgs['LOSS_WEIGHTS']['rcnn_iou_weight']
        return rcnn_loss_iou, {'rcnn_loss_iou': rcnn_loss_iou.detach()}
