"""PointRCNN (pcdet/models/detectors/point_rcnn.py) for kitti_models/pointrcnn.yaml: PointNet2MSG -> PointHeadBox ->
PointRCNNHead, under the reference's module names and order (backbone_3d, point_head, roi_head), so a reference checkpoint
loads with strict=True.  The batch carries `points` (B * N, 1 + 3 + C) [bs_idx, x, y, z, ...] ordered by scene with equally
many rows per scene, and `gt_boxes` (B, M, 8) in training.  Training returns ({'loss': loss_point + loss_rcnn}, tb_dict with the
point_* and rcnn_* entries, disp_dict); eval returns (pred_dicts, recall_dict) with the labels of the first stage's RoIs.

Out of scope: PointNet2Backbone (the reference asserts it off); PointIntraPartOffsetHead belongs to PartA2Net (part_a2_net.py)."""
from .detector3d_template import PointDetector
from .point_head import PointHeadBox
from .pointnet2_backbone import PointNet2MSG
from .pointrcnn_head import PointRCNNHead


class PointRCNN(PointDetector):
    BACKBONE_3D = {'PointNet2MSG': PointNet2MSG}
    POINT_HEAD = {'PointHeadBox': PointHeadBox}
    ROI_HEAD = {'PointRCNNHead': PointRCNNHead}
