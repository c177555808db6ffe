"""VoxelBackBone8x / VoxelResBackBone8x, HeightCompression and SECONDNet on the device against the dense float64 restatement
of the whole stack (tests/golden/sparse_conv_restatement.py dense_backbone: conv3d, the occupancy rule and BatchNorm over the
active rows, on the CPU).

Tolerance: the same dense composition is also run in float32 on the CPU; its error against float64 is measured here, and
the device may be off by 4 times that -- accumulation orders differ in each of up to 12 stacked layers and BatchNorm
amplifies by 1 / sigma.  The figures are max |a - ref| / max |ref|: per dense tensor in eval mode; in train mode for the
loss, over all parameter gradients together (normalised by the largest reference gradient, so that gradients that are zero
in exact arithmetic -- a bias in front of BatchNorm -- count with their absolute noise), and over all running statistics.
Both figures are printed; BASELINE.md section 4 records them."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

from pdanet_amd.config import to_attr
from pdanet_amd.height_compression import HeightCompression
from pdanet_amd.second_net import SECONDNet
from pdanet_amd.spconv_backbone import VoxelBackBone8x, VoxelResBackBone8x

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import sparse_conv_restatement as rs  # noqa: E402

gpu = pytest.mark.gpu
with open(os.path.join(HERE, "golden", "second_state_dict.json")) as _f:
    FIXTURE = json.load(_f)
CFG = FIXTURE['config']
GRID_XYZ, B, COLS, FACTOR = [16, 16, 40], 2, 4, 4.0


def voxels(seed=0, per_scene=400):
    rng = np.random.default_rng(seed)
    nx, ny, nz = GRID_XYZ
    rows = []
    for b in range(B):
        cells = rng.choice(nx * ny * nz, per_scene, replace=False)
        rows.append(np.stack([np.full(per_scene, b), cells // (ny * nx), (cells // nx) % ny, cells % nx], axis=1))
    coords = np.concatenate(rows).astype(np.int32)
    return coords, rng.standard_normal((len(coords), COLS)).astype(np.float32)


def make_backbone(cls, seed=1):
    torch.manual_seed(seed)
    m = cls(to_attr({}), COLS, GRID_XYZ)
    g = torch.Generator().manual_seed(seed + 1)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            with torch.no_grad():
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
                mod.running_mean.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.bias.shape, generator=g) + 0.5)
    return m


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def dense_outputs(model, feats, coords, dtype):
    model = copy.deepcopy(model).to(dtype)
    res = rs.dense_backbone(model, torch.tensor(feats, dtype=dtype), coords, B)
    return model, res


def test_second_net_refuses_other_modules():
    for key, name in (('BACKBONE_3D', 'UNetV2'), ('MAP_TO_BEV', 'PointPillarScatter'), ('VFE', 'PillarVFE'),
                      ('DENSE_HEAD', 'CenterHead')):
        cfg = json.loads(json.dumps(CFG['MODEL']))
        cfg[key]['NAME'] = name
        with pytest.raises(NotImplementedError):
            SECONDNet(to_attr(cfg), 3, CFG['dataset'])
    m = SECONDNet(to_attr(CFG['MODEL']), 3, CFG['dataset'])
    assert [n for n, _ in m.named_children()] == ['vfe', 'backbone_3d', 'map_to_bev_module', 'backbone_2d', 'dense_head']


@gpu
@pytest.mark.parametrize("cls", [VoxelBackBone8x, VoxelResBackBone8x])
def test_gpu_backbone_eval(cls):
    coords, feats = voxels()
    model = make_backbone(cls).eval()
    with torch.no_grad():
        _, ref = dense_outputs(model, feats, coords, torch.float64)
        _, f32 = dense_outputs(model, feats, coords, torch.float32)
        gm = copy.deepcopy(model).cuda()
        out = gm({'voxel_features': torch.from_numpy(feats).cuda(), 'voxel_coords': torch.from_numpy(coords).cuda(), 'batch_size': B})
        got = dict(out['multi_scale_3d_features'], out=out['encoded_spconv_tensor'])
        assert out['encoded_spconv_tensor_stride'] == 8 and out['multi_scale_3d_strides'] == {'x_conv1': 1, 'x_conv2': 2, 'x_conv3': 4, 'x_conv4': 8}
        for name in ('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4', 'out'):
            t = got[name]
            r = ref[name].values.numpy()
            assert t.spatial_shape == list(r.shape[2:]) and t.features.shape[0] == int(ref[name].mask.sum())
            mask = np.zeros(ref[name].mask.shape, bool)
            idx = t.indices.cpu().numpy()
            mask[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = True
            assert np.array_equal(mask, ref[name].mask.numpy())              # the same active sites
            e_dev, e_f32 = rel(t.dense().cpu().numpy(), r), rel(f32[name].values.numpy(), r)
            print(cls.__name__, "eval", name, "device err", e_dev, "float32 CPU err", e_f32)
            assert e_dev <= FACTOR * e_f32, name
        bev = HeightCompression(to_attr({'NUM_BEV_FEATURES': 256}))(out)
        assert bev['spatial_features'].shape == (B, 128 * 2, 2, 2) and bev['spatial_features_stride'] == 8


def dense_train(model, feats, coords, dtype):
    m = copy.deepcopy(model).to(dtype).train()
    res = rs.dense_backbone(m, torch.tensor(feats, dtype=dtype), coords, B)
    loss = (res['out'].rows() ** 2).sum()
    loss.backward()
    return m, float(loss.detach())


def figures(m, loss, ref_m, ref_loss):
    grads = {k: p.grad.detach().cpu().numpy().astype(np.float64) for k, p in m.named_parameters()}
    ref_g = {k: p.grad.numpy() for k, p in ref_m.named_parameters()}
    assert set(grads) == set(ref_g) and all(g is not None for g in grads.values())
    scale = max(np.abs(g).max() for g in ref_g.values())
    e_grad = max(np.abs(grads[k] - ref_g[k]).max() for k in ref_g) / scale
    stats = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.named_buffers() if 'running' in k}
    ref_s = {k: v.numpy() for k, v in ref_m.named_buffers() if 'running' in k}
    s_scale = max(np.abs(v).max() for v in ref_s.values())
    e_stat = max(np.abs(stats[k] - ref_s[k]).max() for k in ref_s) / s_scale
    return abs(loss - ref_loss) / abs(ref_loss), float(e_grad), float(e_stat)


@gpu
@pytest.mark.parametrize("cls", [VoxelBackBone8x, VoxelResBackBone8x])
def test_gpu_backbone_train(cls):
    coords, feats = voxels(seed=2)
    model = make_backbone(cls, seed=5)
    ref_m, ref_loss = dense_train(model, feats, coords, torch.float64)
    f32_m, f32_loss = dense_train(model, feats, coords, torch.float32)
    gm = copy.deepcopy(model).cuda().train()
    out = gm({'voxel_features': torch.from_numpy(feats).cuda(), 'voxel_coords': torch.from_numpy(coords).cuda(), 'batch_size': B})
    loss = (out['encoded_spconv_tensor'].features ** 2).sum()
    loss.backward()
    dev_fig = figures(gm, float(loss.detach()), ref_m, ref_loss)
    f32_fig = figures(f32_m, f32_loss, ref_m, ref_loss)
    for what, d, c in zip(("loss", "gradients", "running statistics"), dev_fig, f32_fig):
        print(cls.__name__, "train", what, "device err", d, "float32 CPU err", c)
    for what, d, c in zip(("loss", "gradients", "running statistics"), dev_fig, f32_fig):
        assert d <= FACTOR * c, what
    assert all(int(v) == 1 for k, v in gm.named_buffers() if k.endswith('num_batches_tracked'))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@gpu
def test_gpu_second_net_train_and_eval():
    from pdanet_amd.voxel_utils import VoxelGenerator, collate_voxels
    ds = CFG['dataset']
    torch.manual_seed(3)
    model = SECONDNet(to_attr(CFG['MODEL']), 3, ds).cuda()
    rng = np.random.default_rng(5)
    pcr = np.array(ds['point_cloud_range'], np.float64)
    counts = [1500, 900]                                       # a ragged scene pair
    pts = np.concatenate([np.concatenate([rng.uniform(pcr[:3], pcr[3:], (n, 3)), rng.random((n, 1))], axis=1) for n in counts])
    offs = torch.tensor([0, counts[0], sum(counts)], dtype=torch.int64).cuda()
    gen = VoxelGenerator(ds['voxel_size'], ds['point_cloud_range'], 4, 5, 2000)
    voxels_, coords, num_points = collate_voxels(*gen.generate_batch((dev(pts.astype(np.float32)), offs, max(counts))))
    assert coords.shape[1] == 4 and int(coords[:, 0].max()) == 1 and voxels_.shape[1:] == (5, 4)
    gt = np.zeros((B, 3, 8), np.float32)
    gt[0, 0] = [0.4, 0.0, -1.0, 3.9, 1.6, 1.56, 0.3, 1]
    gt[0, 1] = [0.3, 0.1, -0.6, 0.8, 0.6, 1.73, 1.2, 2]
    gt[1, 0] = [0.5, -0.1, -0.6, 1.76, 0.6, 1.73, -0.4, 3]
    batch = {'voxels': voxels_, 'voxel_coords': coords, 'voxel_num_points': num_points, 'gt_boxes': dev(gt), 'batch_size': B}
    model.train()
    ret, tb, disp = model(dict(batch))
    assert torch.isfinite(ret['loss']) and disp == {}
    assert set(tb) == {'loss_rpn', 'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir', 'rpn_loss'}
    ret['loss'].backward()
    for name, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    model.eval()
    with torch.no_grad():
        pred_dicts, recall = model(dict(batch))
    assert len(pred_dicts) == B and set(pred_dicts[0]) == {'pred_boxes', 'pred_scores', 'pred_labels'}
    assert set(recall) == {'gt', 'roi_0.3', 'rcnn_0.3', 'roi_0.5', 'rcnn_0.5', 'roi_0.7', 'rcnn_0.7'}
    own = model.state_dict()
    assert [[k, list(v.shape)] for k, v in own.items()] == FIXTURE['SECONDNet']
    sd = {k: torch.zeros(shape, dtype=own[k].dtype) for k, shape in FIXTURE['SECONDNet']}
    fresh = SECONDNet(to_attr(CFG['MODEL']), 3, ds).cuda()
    fresh.load_state_dict(sd, strict=True)
