"""The anchor-based nuScenes detectors (pcdet/models/detectors/pointpillar.py and second_net.py under
nuscenes_models/cbgs_pp_multihead.yaml and cbgs_second_multihead.yaml): ten classes in six heads of AnchorHeadMulti with
BOX_CODER_CONFIG {code_size: 9, encode_angle_by_sincos: True}, WeightedL1Loss on ten code columns, MULTI_CLASSES_NMS.

PointPillarMultiHead   PillarVFE -> PointPillarScatter -> BaseBEVBackbone -> AnchorHeadMultiCoded
SECONDNetMultiHead     MeanVFE -> VoxelBackBone8x / VoxelResBackBone8x -> HeightCompression -> BaseBEVBackbone ->
                       AnchorHeadMultiCoded; a padded batch (voxel_utils.collate_voxels_padded) runs without a host read.

Both under the reference's module names (vfe, backbone_3d, map_to_bev_module, backbone_2d, dense_head), so a reference checkpoint
loads with strict=True; the yaml's DENSE_HEAD.NAME `AnchorHeadMulti` (or `AnchorHeadSingle`) names the coded head here, which
also takes the plain 7-column code.  pointpillar.PointPillar and second_net.SECONDNet keep their 7-column heads.  The batch
carries gt_boxes (B, M, 10): the box, two velocity columns (NaN where unknown), the 1-based label.  Training returns
({'loss': loss}, tb_dict, disp_dict) with 0-dim device tensors in tb_dict; eval returns (pred_dicts, recall_dict) with pred_boxes
(n, 9).  build() picks the class by MODEL.NAME."""
from .anchor_head_coded import AnchorHeadMultiCoded, AnchorHeadSingleCoded
from .detector3d_template import PillarDetector, VoxelDetector
from .mean_vfe import MeanVFE
from .pillar_vfe import PillarVFE
from .spconv_backbone import VoxelBackBone8x, VoxelResBackBone8x

DENSE_HEAD = {'AnchorHeadMulti': AnchorHeadMultiCoded, 'AnchorHeadSingle': AnchorHeadSingleCoded}


class PointPillarMultiHead(PillarDetector):
    VFE = {'PillarVFE': PillarVFE}
    DENSE_HEAD = DENSE_HEAD


class SECONDNetMultiHead(VoxelDetector):
    VFE = {'MeanVFE': MeanVFE}
    BACKBONE_3D = {'VoxelBackBone8x': VoxelBackBone8x, 'VoxelResBackBone8x': VoxelResBackBone8x}
    DENSE_HEAD = DENSE_HEAD


DETECTORS = {'PointPillar': PointPillarMultiHead, 'SECONDNet': SECONDNetMultiHead}


def build(model_cfg, num_class, dataset):
    """The detector of a model config by its NAME: PointPillar or SECONDNet."""
    if model_cfg['NAME'] not in DETECTORS:
        raise NotImplementedError("MODEL.NAME %r (%s)" % (model_cfg['NAME'], ", ".join(DETECTORS)))
    return DETECTORS[model_cfg['NAME']](model_cfg, num_class, dataset)
