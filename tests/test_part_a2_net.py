"""PartA2Net (pdanet_amd/part_a2_net.py): the state dict and child order of the reference's detector for kitti_models/PartA2.yaml
(tests/golden/parta2_state_dict.json, make_parta2_golden.py), its refusals, and one training iteration and one eval pass on a
tiny grid: MeanVFE -> UNetV2 -> HeightCompression -> BaseBEVBackbone -> AnchorHeadSingle -> PointIntraPartOffsetHead ->
PartA2FCHead."""
import json
import os

import numpy as np
import pytest
import torch

from pdanet_amd.config import to_attr
from pdanet_amd.part_a2_net import PartA2Net
from pdanet_amd.part_head import PointIntraPartOffsetHead
from pdanet_amd.parta2_head import PartA2FCHead
from pdanet_amd.spconv_unet import UNetV2

HERE = os.path.dirname(os.path.abspath(__file__))
gpu = pytest.mark.gpu
with open(os.path.join(HERE, "golden", "parta2_state_dict.json")) as _f:
    FIXTURE = json.load(_f)
CFG = FIXTURE['config']
B = 2


def model_cfg(**blocks):
    cfg = json.loads(json.dumps(CFG['MODEL']))
    for key, value in blocks.items():
        if value is None:
            cfg.pop(key)
        else:
            cfg[key].update(value)
    return cfg


def tiny_model_cfg():
    cfg = model_cfg(BACKBONE_2D={'LAYER_NUMS': [1, 1]},
                    ROI_HEAD={'SHARED_FC': [32], 'CLS_FC': [32], 'REG_FC': [32], 'DP_RATIO': 0,
                              'ROI_AWARE_POOL': {'POOL_SIZE': 4, 'NUM_FEATURES': 32, 'MAX_POINTS_PER_VOXEL': 16}})
    cfg['ROI_HEAD']['TARGET_CONFIG']['ROI_PER_IMAGE'] = 16
    for mode, post in (('TRAIN', 32), ('TEST', 16)):
        cfg['ROI_HEAD']['NMS_CONFIG'][mode].update(NMS_PRE_MAXSIZE=256, NMS_POST_MAXSIZE=post)
    return cfg


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_state_dict_and_child_order_are_the_references():
    m = PartA2Net(to_attr(CFG['MODEL']), 3, CFG['dataset'])
    own = m.state_dict()
    assert [[k, list(v.shape)] for k, v in own.items()] == FIXTURE['PartA2Net']
    assert [n for n, _ in m.named_children()] == FIXTURE['PartA2Net_children']
    assert [type(x) for x in m.module_list[-2:]] == [PointIntraPartOffsetHead, PartA2FCHead] and len(m.module_list) == 7
    assert isinstance(m.backbone_3d, UNetV2) and m.dense_head.predict_boxes_when_training and not hasattr(m, 'pfe')
    assert m.point_head.num_class == 1 and m.roi_head.num_class == 1 and m.model_cfg is not None and 'ROI_HEAD' in m.model_cfg
    m.load_state_dict({k: torch.zeros(shape, dtype=own[k].dtype) for k, shape in FIXTURE['PartA2Net']}, strict=True)


def test_no_block_of_the_config_is_modified():
    cfg = model_cfg()
    before = json.dumps(cfg, sort_keys=True)
    PartA2Net(to_attr(cfg), 3, CFG['dataset'])
    assert json.dumps(cfg, sort_keys=True) == before


def test_other_names_and_the_anchor_free_form_are_refused():
    for key, name in (('VFE', 'PillarVFE'), ('BACKBONE_3D', 'VoxelBackBone8x'), ('MAP_TO_BEV', 'PointPillarScatter'),
                      ('DENSE_HEAD', 'CenterHead'), ('POINT_HEAD', 'PointHeadSimple'), ('POINT_HEAD', 'PointHeadBox'),
                      ('ROI_HEAD', 'PVRCNNHead'), ('ROI_HEAD', 'VoxelRCNNHead')):
        with pytest.raises(NotImplementedError):
            PartA2Net(to_attr(model_cfg(**{key: {'NAME': name}})), 3, CFG['dataset'])
    with pytest.raises(NotImplementedError, match="PartA2_free"):
        PartA2Net(to_attr(model_cfg(DENSE_HEAD=None)), 3, CFG['dataset'])
    cfg = model_cfg()
    cfg['PFE'] = {'NAME': 'VoxelSetAbstraction'}
    with pytest.raises(NotImplementedError):
        PartA2Net(to_attr(cfg), 3, CFG['dataset'])
    for key in ('POINT_HEAD', 'ROI_HEAD'):
        with pytest.raises(ValueError, match=key):
            PartA2Net(to_attr(model_cfg(**{key: None})), 3, CFG['dataset'])


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def tiny_batch():
    from pdanet_amd.voxel_utils import VoxelGenerator, collate_voxels
    ds = CFG['dataset']
    rng = np.random.default_rng(5)
    pcr = np.array(ds['point_cloud_range'], np.float64)
    gt = np.zeros((B, 3, 8), np.float32)
    gt[0, 0] = [0.4, 0.0, -1.0, 0.5, 0.3, 1.5, 0.3, 1]
    gt[0, 1] = [0.2, 0.2, -0.6, 0.2, 0.2, 1.7, 1.2, 2]
    gt[1, 0] = [0.5, -0.1, -0.6, 0.4, 0.3, 1.7, -0.4, 3]
    counts = [1500, 900]                                       # a ragged scene pair
    pts = np.concatenate([np.concatenate([rng.uniform(pcr[:3], pcr[3:], (n, 3)), rng.random((n, 1))], axis=1) for n in counts])
    offs = torch.tensor([0, counts[0], sum(counts)], dtype=torch.int64).cuda()
    gen = VoxelGenerator(ds['voxel_size'], ds['point_cloud_range'], 4, 5, 2000)
    voxels, coords, num_points = collate_voxels(*gen.generate_batch((dev(pts.astype(np.float32)), offs, max(counts))))
    return {'voxels': voxels, 'voxel_coords': coords, 'voxel_num_points': num_points, 'gt_boxes': dev(gt), 'batch_size': B,
            'roi_target_seed': 11}


@gpu
def test_gpu_training_iteration_and_eval():
    torch.manual_seed(3)
    model = PartA2Net(to_attr(tiny_model_cfg()), 3, CFG['dataset']).cuda()
    batch = tiny_batch()
    model.train()
    ret, tb, disp = model(dict(batch))
    assert torch.isfinite(ret['loss']) and disp == {}
    for key in ('rpn_loss', 'point_loss_cls', 'point_loss_part', 'rcnn_loss_cls', 'rcnn_loss_reg'):
        assert key in tb and torch.isfinite(torch.as_tensor(tb[key])).all(), key
    ret['loss'].backward()
    for name, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    # the labels of the voxel centres: every kind occurs, so the part loss saw foreground
    labels = model.point_head.forward_ret_dict['point_cls_labels']
    assert labels.shape[0] == batch['voxel_coords'].shape[0] and (labels > 0).any() and (labels == 0).any()
    assert float(tb['point_loss_part']) > 0
    with pytest.raises(NotImplementedError, match="padded"):
        model(dict(batch, voxel_num_active=torch.tensor([1], dtype=torch.int32, device='cuda')))
    model.eval()
    with torch.no_grad():
        pred_dicts, recall = model(dict(batch))
    assert len(pred_dicts) == B and set(pred_dicts[0]) == {'pred_boxes', 'pred_scores', 'pred_labels'}
    assert set(recall) == {'gt', 'roi_0.3', 'rcnn_0.3', 'roi_0.5', 'rcnn_0.5', 'roi_0.7', 'rcnn_0.7'}
    assert all(torch.isfinite(d['pred_boxes']).all() for d in pred_dicts)
