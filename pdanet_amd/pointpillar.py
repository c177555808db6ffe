"""PointPillar (pcdet/models/detectors/pointpillar.py) for kitti_models/pointpillar.yaml, pointpillar_newaugs.yaml and
waymo_models/pointpillar_1x.yaml: PillarVFE -> PointPillarScatter -> BaseBEVBackbone -> AnchorHeadSingle, under the
reference's module names (vfe, map_to_bev_module, backbone_2d, dense_head), so a reference checkpoint loads with
strict=True.  The batch carries the collated hard voxels (voxel_utils.VoxelGenerator.generate_batch + collate_voxels).
Training returns ({'loss': loss}, tb_dict, disp_dict) with 0-dim device tensors in tb_dict; eval returns what
model_nms_utils.to_pred_and_recall_dicts returns, after one host read for predictions and recall."""
from .anchor_head import AnchorHeadSingle
from .detector3d_template import PillarDetector
from .pillar_vfe import PillarVFE


class PointPillar(PillarDetector):
    VFE = {'PillarVFE': PillarVFE}
    DENSE_HEAD = {'AnchorHeadSingle': AnchorHeadSingle}
