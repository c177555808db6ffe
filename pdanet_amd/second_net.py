"""SECONDNet (pcdet/models/detectors/second_net.py) for kitti_models/second.yaml, second_multihead.yaml and
waymo_models/second.yaml: MeanVFE -> VoxelBackBone8x / VoxelResBackBone8x -> HeightCompression -> BaseBEVBackbone ->
AnchorHeadSingle / AnchorHeadMulti (whose list of per-head scores takes MULTI_CLASSES_NMS), under the reference's
module names (vfe, backbone_3d, map_to_bev_module, backbone_2d, dense_head), so a reference checkpoint (spconv 2.x) loads
with strict=True.  The batch carries the collated hard voxels (voxel_utils.VoxelGenerator.generate_batch + collate_voxels).
Training returns ({'loss': loss}, tb_dict, disp_dict); eval returns what PointPillar returns."""
from .anchor_head import AnchorHeadSingle
from .anchor_head_multi import AnchorHeadMulti
from .detector3d_template import VoxelDetector
from .mean_vfe import MeanVFE
from .spconv_backbone import VoxelBackBone8x, VoxelResBackBone8x


class SECONDNet(VoxelDetector):
    VFE = {'MeanVFE': MeanVFE}
    BACKBONE_3D = {'VoxelBackBone8x': VoxelBackBone8x, 'VoxelResBackBone8x': VoxelResBackBone8x}
    DENSE_HEAD = {'AnchorHeadSingle': AnchorHeadSingle, 'AnchorHeadMulti': AnchorHeadMulti}
