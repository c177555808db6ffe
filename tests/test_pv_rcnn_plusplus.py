"""PV-RCNN++: the RoI point filter and sectorized proposal-centric sampling (csrc/spc_sample.hip, voxel_set_abstraction_spc.py),
the VectorPool layers (vector_pool_modules.py) and the detector (pv_rcnn_plusplus.py) against the reference's own CPU run
(tests/golden/pv_rcnn_plusplus.npz and pv_rcnn_plusplus_state_dicts.json, made by make_pv_rcnn_plusplus_golden.py).

Decisions -- mask, sector keys, segment counts, keypoints -- must equal the fixture exactly: the generator constructed the inputs
with margins (no point within 1e-4 of its keep threshold, no two candidate RoIs within 1e-5, no kept point within 1e-4 rad of a
sector boundary) under which float32 on any platform decides as float64 does.

Values follow the project's 4x rule (tests/test_pv_rcnn.py): the fixture holds the reference's float32 CPU run next to the same
run in float64; the device may differ from float64 by at most 4 times what the float32 CPU run does.  Figures are
max |a - ref| / max |ref| per tensor, all parameter gradients together normalised by the largest reference gradient.  Every
figure is printed.  For the parameter gradients of the three MSG modules -- float32 sums over the 70 keypoints -- the reference's
figure is the largest over nine float32 CPU runs that differ in the order of the keypoints only (grad_params_err_orders, recorded
by the generator): one order is one sample of that sum's rounding error, and for local_interpolation the first order's sample is
5.2e-8, below a single float32 rounding, where the nine orders reach 3.3e-7.

Measured on an MI355X (device / float32 CPU): interpolation rows 6.6e-8 .. 1.1e-7 / 7.4e-8 .. 1.1e-7, bitwise the composed path's;
their gradient 1.5e-7 .. 2.5e-7 / 1.8e-7 .. 2.6e-7; the three MSG modules' outputs 9.3e-8 .. 1.4e-7 / 8.4e-8 .. 1.5e-7, parameter
gradients 1.9e-7 .. 2.5e-7 / 3.3e-7 .. 5.2e-7; the SPC VoxelSetAbstraction 1.2e-7 .. 3.8e-7 / 1.4e-7 .. 4.0e-7; the ragged point head's
loss 5.7e-8 / 5.7e-8; the head's loss and tb_dict 3.3e-8 .. 2.5e-7 / 3.3e-8 .. 5.3e-7 (BASELINE.md has the table)."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

from pdanet_amd.config import to_attr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import pv_rcnn_plusplus_restatement as pp  # noqa: E402

gpu = pytest.mark.gpu
FACTOR = 4.0
PCR, VOXEL = [0.0, -4.0, -2.0, 8.0, 4.0, 2.0], [0.25, 0.25, 0.25]            # the geometry of the vsa_* fixture
with open(os.path.join(HERE, "golden", "pv_rcnn_plusplus_state_dicts.json")) as _f:
    FIXTURE = json.load(_f)
YAMLS = ("pv_rcnn_plusplus", "pv_rcnn_plusplus_resnet")


@pytest.fixture(scope="module")
def npz():
    with np.load(os.path.join(HERE, "golden", "pv_rcnn_plusplus.npz")) as f:
        return {k: f[k] for k in f.files}


def sub(npz, prefix):
    return {k[len(prefix):]: v for k, v in npz.items() if k.startswith(prefix)}


def layout(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def msg_cfg(npz, kind):
    return json.loads(str(npz["msg_%s_cfg" % kind]))


# ---- without a GPU --------------------------------------------------------------------------------------------------------
def test_new_symbols_exist():
    from pdanet_amd import _lib, build
    build.build()
    lib = _lib.load()
    for name in ("pda_roi_point_filter", "pda_vector_interp_fwd", "pda_vector_interp_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.pda_abi_version() == 20


def test_state_dict_layouts_are_the_references(npz):
    from pdanet_amd import vector_pool_modules as vp
    from pdanet_amd.pv_rcnn_plusplus import PVRCNNPlusPlusHead
    from pdanet_amd.voxel_set_abstraction_spc import VoxelSetAbstractionSPC
    before = json.dumps(FIXTURE, sort_keys=True)
    mlp = [8, 16, 16]
    assert layout(vp.VectorPoolLocalInterpolateModule(mlp=mlp, num_voxels=[3, 3, 3], max_neighbour_distance=1.0, nsample=-1,
                                                      neighbor_type=0)) == FIXTURE['VectorPoolLocalInterpolateModule']
    assert mlp == [8, 16, 16]                                                     # the caller's list stays as it is
    assert layout(vp.VectorPoolAggregationModule(input_channels=8, num_reduced_channels=4, num_channels_of_local_aggregation=4,
                                                 post_mlps=(8, 8), max_neighbor_distance=1.0)) == FIXTURE['VectorPoolAggregationModule']
    msg = vp.VectorPoolAggregationModuleMSG(input_channels=8, config=to_attr(msg_cfg(npz, 'voxel_random_choice')))
    assert layout(msg) == FIXTURE['VectorPoolAggregationModuleMSG']
    cfg, ds = FIXTURE['config']['pv_rcnn_plusplus'], FIXTURE['dataset']
    vsa = VoxelSetAbstractionSPC(to_attr(cfg['PFE']), ds['voxel_size'], ds['point_cloud_range'],
                                 num_bev_features=cfg['MAP_TO_BEV']['NUM_BEV_FEATURES'], num_rawpoint_features=ds['num_point_features'])
    assert layout(vsa) == FIXTURE['VoxelSetAbstraction']
    head = PVRCNNPlusPlusHead(input_channels=vsa.num_point_features, model_cfg=to_attr(cfg['ROI_HEAD']), num_class=1)
    assert layout(head) == FIXTURE['PVRCNNHead']
    assert json.dumps(FIXTURE, sort_keys=True) == before                          # no module modified its config


@pytest.mark.parametrize("name", YAMLS)
def test_both_yamls_construct_and_load_a_reference_checkpoint(name):
    from pdanet_amd import pv_rcnn_plusplus
    cfg = to_attr(copy.deepcopy(FIXTURE['config'][name]))
    model = pv_rcnn_plusplus.build(cfg, 3, FIXTURE['dataset'])
    own = model.state_dict()
    assert [[k, list(v.shape)] for k, v in own.items()] == FIXTURE[name]
    assert [n for n, _ in model.named_children()] == ['vfe', 'backbone_3d', 'map_to_bev_module', 'pfe', 'backbone_2d', 'dense_head',
                                                      'point_head', 'roi_head']
    model.load_state_dict({k: torch.zeros(shape, dtype=own[k].dtype) for k, shape in FIXTURE[name]}, strict=True)
    assert json.dumps(cfg, sort_keys=True) == json.dumps(FIXTURE['config'][name], sort_keys=True)


def test_the_old_modules_still_refuse_and_the_new_ones_refuse_what_is_not_built(npz):
    from pdanet_amd import pointnet2_stack_modules, vector_pool_modules
    from pdanet_amd.pv_rcnn_plusplus import PVRCNNPlusPlus, build
    from pdanet_amd.pvrcnn_head import PVRCNNHead
    from pdanet_amd.voxel_set_abstraction import VoxelSetAbstraction
    from pdanet_amd.voxel_set_abstraction_spc import VoxelSetAbstractionSPC
    cfg, ds = FIXTURE['config']['pv_rcnn_plusplus'], FIXTURE['dataset']
    make = lambda cls, pfe: cls(to_attr(pfe), ds['voxel_size'], ds['point_cloud_range'], num_bev_features=256, num_rawpoint_features=5)
    with pytest.raises(NotImplementedError, match="SPC is PV-RCNN\\+\\+"):
        make(VoxelSetAbstraction, cfg['PFE'])
    fps = copy.deepcopy(cfg['PFE'])
    fps['SAMPLE_METHOD'] = 'FPS'
    with pytest.raises(NotImplementedError, match="FILTER_NEIGHBOR_WITH_ROI"):
        make(VoxelSetAbstraction, fps)
    with pytest.raises(NotImplementedError, match="not part of this project"):
        pointnet2_stack_modules.build_local_aggregation_module(64, to_attr(cfg['PFE']['SA_LAYER']['x_conv3']))
    with pytest.raises(NotImplementedError):
        PVRCNNHead(input_channels=90, model_cfg=to_attr(cfg['ROI_HEAD']), num_class=1)
    other = copy.deepcopy(cfg['PFE'])
    other['POINT_SOURCE'] = 'voxels'
    with pytest.raises(NotImplementedError, match="POINT_SOURCE"):
        make(VoxelSetAbstractionSPC, other)
    with pytest.raises(NotImplementedError, match="xyz_encoding_type"):
        vector_pool_modules.VectorPoolLocalInterpolateModule(None, [2, 2, 2], 1.0, -1, 0, xyz_encoding_type='pos')
    with pytest.raises(NotImplementedError, match="MODEL.NAME"):
        build(to_attr(dict(cfg, NAME='PVRCNN')), 3, ds)
    model = PVRCNNPlusPlus(to_attr(copy.deepcopy(cfg)), 3, ds)
    with pytest.raises(NotImplementedError, match="padded batch"):
        model({'voxel_num_active': torch.zeros(1), 'batch_size': 2})
    # the layers the new builder adds to the old one's
    sa = {'MLPS': [[16, 16]], 'POOL_RADIUS': [0.4], 'NSAMPLE': [16]}
    assert isinstance(vector_pool_modules.build_local_aggregation_module(4, sa)[0], pointnet2_stack_modules.StackSAModuleMSG)


def test_quotas_are_the_references(npz):
    from pdanet_amd.voxel_set_abstraction_spc import sector_quotas
    for tag in "ab":
        for seg, quota, mask_cnt in zip(npz["spc_seg_" + tag], npz["spc_quota_" + tag], kept_per_scene(npz, tag)):
            if mask_cnt:
                assert sector_quotas(seg.tolist(), mask_cnt, int(npz["spc_settings"][2])) == quota.tolist()


def kept_per_scene(npz, tag):
    counts = npz["spc_counts"].tolist()
    mask = npz["spc_mask_" + tag]
    return [int(mask[:counts[0]].sum()), int(mask[counts[0]:].sum())]


# ---- the figures of the 4x rule -----------------------------------------------------------------------------------------------
def rel(a, ref):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def together(got, ref):
    assert set(got) == set(ref), set(got) ^ set(ref)
    scale = max(float(np.abs(np.asarray(r, np.float64)).max()) for r in ref.values())
    return max(float(np.abs(np.asarray(got[k], np.float64) - np.asarray(ref[k], np.float64)).max()) for k in ref) / scale


def check(what, e_dev, e_gold):
    print("%s: device %.3e, reference in float32 on the CPU %.3e, ratio %.2f" % (what, e_dev, e_gold, e_dev / max(e_gold, 1e-300)))
    assert e_dev <= FACTOR * e_gold, what


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def param_grads(fix, suffix):
    """{name: gradient} of the fixture's 'grad.<parameter>' entries, float32 ('') or float64 ('_f64')"""
    names = [k for k in fix if k.startswith("grad.") and not k.endswith("_f64")]
    return {k[5:]: fix[k + suffix] for k in names}


def check_module_run(what, fix, outputs, extra_grads, module, param_gold=None):
    """outputs / extra_grads: {name: device tensor} against fix[name] / fix['grad_' + name] and their _f64 twins; the parameter
    gradients of `module` together, against param_gold when given (else the fixture's one float32 run)."""
    for k, v in outputs.items():
        check("%s %s" % (what, k), rel(v, fix[k + "_f64"]), rel(fix[k], fix[k + "_f64"]))
    for k, v in extra_grads.items():
        check("%s d %s" % (what, k), rel(v, fix["grad_" + k + "_f64"]), rel(fix["grad_" + k], fix["grad_" + k + "_f64"]))
    got = {k: p.grad.detach().cpu().numpy() for k, p in module.named_parameters()}
    e_gold = together(param_grads(fix, ""), param_grads(fix, "_f64")) if param_gold is None else param_gold
    check("%s parameter gradients" % what, together(got, param_grads(fix, "_f64")), e_gold)


# ---- filter and SPC ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("tag", ["a", "b"])
def test_gpu_filter_and_spc_equal_the_reference(npz, tag):
    """Configuration a: 6 RoIs (two zero rows), every sector of scene 0 filled, sector 2 of scene 1 empty, quotas that round up;
    configuration b: scene 1 keeps nothing and contributes its first point."""
    from pdanet_amd.voxel_set_abstraction_spc import sample_points_with_roi, sector_fps
    radius, S, K = float(npz["spc_settings"][0]), int(npz["spc_settings"][1]), int(npz["spc_settings"][2])
    points, counts, rois = dev(npz["spc_points"]), dev(npz["spc_counts"]), dev(npz["spc_rois_" + tag])
    mask, keys = sample_points_with_roi(rois, points, counts, radius, num_sectors=S)
    assert mask.dtype == torch.uint8 and keys.dtype == torch.int32
    assert np.array_equal(mask.cpu().numpy(), npz["spc_mask_" + tag])
    assert np.array_equal(keys.cpu().numpy(), npz["spc_keys_" + tag])
    only_mask, no_keys = sample_points_with_roi(rois, points, counts, radius)
    assert no_keys is None and torch.equal(only_mask, mask)
    seg = torch.bincount(keys.long(), minlength=2 * (S + 1)).view(2, S + 1)[:, :S]
    assert np.array_equal(seg.cpu().numpy(), npz["spc_seg_" + tag])
    rows, per_scene = sector_fps(points, mask, keys, 2, K, S)
    want = npz["spc_keypoints_" + tag]
    assert per_scene == [int((want[:, 0] == b).sum()) for b in range(2)]
    assert np.array_equal(points[rows].cpu().numpy(), want[:, 1:4])


@gpu
@pytest.mark.parametrize("n0, n1", [(1536, 1300), (1700, 1280), (1, 1300), (1700, 0), (255, 257)])
def test_gpu_filter_does_not_depend_on_the_tiling(npz, n0, n1):
    """The first n0 points of scene 0 and the first n1 of scene 1: multiples of the 256-point tile and not, tiles that end at the
    scene boundary and tiles that would straddle it, an empty scene."""
    from pdanet_amd.voxel_set_abstraction_spc import sample_points_with_roi
    c0 = int(npz["spc_counts"][0])
    take = np.concatenate([np.arange(n0), c0 + np.arange(n1)])
    guard = torch.full((len(take) + 300,), 7, dtype=torch.float32, device='cuda').repeat(3, 1).t().contiguous()
    guard[:len(take)] = dev(npz["spc_points"][take])
    mask, keys = sample_points_with_roi(dev(npz["spc_rois_a"]), guard, dev(np.array([n0, n1], np.int32)), float(npz["spc_settings"][0]),
                                        num_sectors=6)
    assert np.array_equal(mask[:len(take)].cpu().numpy(), npz["spc_mask_a"][take])
    assert np.array_equal(keys[:len(take)].cpu().numpy(), npz["spc_keys_a"][take])
    assert not mask[len(take):].any()                                              # rows past the counts: not kept, of no scene
    assert bool((keys[len(take):] == 2 * 7).all())
    from pdanet_amd.voxel_set_abstraction_spc import sector_fps
    with pytest.raises(ValueError, match="past the per-scene counts"):
        sector_fps(guard, mask, keys, 2, 64, 6)


@gpu
def test_gpu_filter_without_rois_or_points(npz):
    from pdanet_amd.voxel_set_abstraction_spc import sample_points_with_roi
    points, counts = dev(npz["spc_points"]), dev(npz["spc_counts"])
    mask, keys = sample_points_with_roi(torch.zeros((2, 0, 7), device='cuda'), points, counts, 1.6, num_sectors=6)
    assert not mask.any() and np.array_equal(keys.cpu().numpy(), np.repeat([6, 13], npz["spc_counts"]))
    mask, _ = sample_points_with_roi(dev(npz["spc_rois_a"]), points[:0], torch.zeros(2, dtype=torch.int32, device='cuda'), 1.6)
    assert mask.shape == (0,)


# ---- the fused interpolation rows ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c, g", [(2, 8), (2, 27), (32, 8), (32, 27)])
def test_gpu_fused_interpolation_rows(npz, c, g, monkeypatch):
    """M = 70 centres in two scenes, scene 1 without support points, cells without neighbour in scene 0."""
    from pdanet_amd import vector_pool_modules as vp
    tag = "interp_c%d_g%d_" % (c, g)
    side, dist = round(g ** (1 / 3)), float(npz[tag + "dist"])
    xyz, new_xyz = dev(npz["interp_xyz"]), dev(npz["interp_new_xyz"])
    xyz_cnt, new_cnt = dev(npz["interp_xyz_cnt"]), dev(npz["interp_new_cnt"])
    mod = vp.VectorPoolLocalInterpolateModule(mlp=None, num_voxels=[side] * 3, max_neighbour_distance=dist, nsample=-1, neighbor_type=0,
                                              neighbour_distance_multiplier=2.0)
    centers = vp.VectorPoolAggregationModule.get_dense_voxels_by_center(new_xyz, dist, [side] * 3)
    grad_out = dev(pp.interp_grad_out(70 * g, c + 9))
    got = {}
    for path in ("fused", "composed"):
        monkeypatch.setenv(vp.ENV, path)
        f = dev(npz["interp_feat_c%d" % c]).requires_grad_(True)
        rows = mod(xyz, f, xyz_cnt, new_xyz, centers, new_cnt)
        assert rows.shape == (70 * g, c + 9)
        (rows * grad_out).sum().backward()
        got[path] = (rows.detach(), f.grad)
    _, idx, _ = vp.pointnet2_utils.three_nn_for_vector_pool_by_two_step(xyz, xyz_cnt, new_xyz, centers, new_cnt, dist, -1, 0, 1000, g, 2.0)
    empty = (idx[..., 0] < 0).cpu().numpy()
    assert empty[40:].all() and empty[:40].any() and not empty[:40].all()
    assert not got["fused"][0].view(70, g, -1)[torch.from_numpy(empty).cuda()].any()
    f64 = torch.from_numpy(npz["interp_feat_c%d" % c]).double().requires_grad_(True)
    truth = pp.interp_rows(xyz.cpu(), f64, centers.cpu(), idx.cpu())
    (truth * grad_out.cpu().double().view(70, -1)).sum().backward()
    truth = truth.detach().numpy().reshape(-1, c + 9)
    print("%s fused against composed on the device: rows %.3e, gradient %.3e" % (
        tag, rel(got["fused"][0], got["composed"][0].cpu().numpy()), rel(got["fused"][1], got["composed"][1].cpu().numpy())))
    for path in ("fused", "composed"):
        check(tag + path + " rows", rel(got[path][0], truth), float(npz[tag + "rows_err"]))
        check(tag + path + " d features", rel(got[path][1], f64.grad.numpy()), rel(npz[tag + "grad"], f64.grad.numpy()))
    assert torch.equal(got["fused"][0], got["composed"][0])                        # the forward: the same bits


# ---- modules -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind, path", [("local_interpolation", "fused"), ("local_interpolation", "composed"),
                                        ("voxel_avg_pool", "fused"), ("voxel_random_choice", "fused")])
def test_gpu_vector_pool_msg_against_the_reference(npz, kind, path, monkeypatch):
    from pdanet_amd import vector_pool_modules as vp
    monkeypatch.setenv(vp.ENV, path)
    fix = sub(npz, "msg_%s_" % kind)
    mod = vp.VectorPoolAggregationModuleMSG(input_channels=8, config=to_attr(msg_cfg(npz, kind)))
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in sub(fix, "sd.").items()}, strict=True)
    mod = mod.cuda().train()
    f = dev(fix["features"]).requires_grad_(True)
    new_xyz, out = mod(xyz=dev(fix["xyz"]), xyz_batch_cnt=dev(fix["xyz_cnt"]), new_xyz=dev(fix["new_xyz"]),
                       new_xyz_batch_cnt=dev(fix["new_cnt"]), features=f)
    (out * dev(fix["grad_out"])).sum().backward()
    check_module_run("msg %s %s" % (kind, path), fix, {"out": out}, {"features": f.grad}, mod,
                     param_gold=float(fix["grad_params_err_orders"]))
    assert mod.layer_0.num_mean_points_per_grid >= 20 and (mod.layer_0.local_interpolate_module is None) == (kind != "local_interpolation")


def vsa_batch(npz, device):
    import types
    to = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device))
    f, m = to(npz["vsa_x_conv2_features"]).requires_grad_(True), to(npz["vsa_bev"]).requires_grad_(True)
    return {'batch_size': 2, 'points': to(npz["vsa_points"]), 'rois': to(npz["vsa_rois"]), 'spatial_features': m, 'spatial_features_stride': 4,
            'multi_scale_3d_features': {'x_conv2': types.SimpleNamespace(indices=to(npz["vsa_x_conv2_indices"]), features=f)}}, f, m


@gpu
def test_gpu_spc_voxel_set_abstraction_against_the_reference(npz):
    """SPC keypoints (exact), bev + RoI-filtered x_conv2 + RoI-filtered raw_points through VectorPool layers, forward and backward."""
    from pdanet_amd.voxel_set_abstraction_spc import VoxelSetAbstractionSPC
    fix = sub(npz, "vsa_")
    mod = VoxelSetAbstractionSPC(to_attr(json.loads(str(npz["vsa_cfg"]))), VOXEL, PCR, num_bev_features=npz["vsa_bev"].shape[1],
                                 num_rawpoint_features=4)
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in sub(fix, "sd.").items()}, strict=True)
    mod = mod.cuda().train()
    batch, f, m = vsa_batch(npz, 'cuda')
    bd = mod(batch)
    assert np.array_equal(bd['point_coords'].cpu().numpy(), fix["point_coords"])
    loss = (bd['point_features'] * dev(fix["grad_after"])).sum() + (bd['point_features_before_fusion'] * dev(fix["grad_before"])).sum()
    loss.backward()
    check_module_run("vsa", fix, {"before_fusion": bd['point_features_before_fusion'], "point_features": bd['point_features']},
                     {"x_conv2": f.grad, "bev": m.grad}, mod)


@gpu
def test_gpu_a_scene_whose_filter_keeps_no_row_pools_zeros(npz):
    """Scene 1's RoIs moved far away: its keypoint is its first point, no row of either source survives there, and the pooled
    features of that keypoint are the layers' response to an all-zero input; scene 0 is what it was."""
    from pdanet_amd.voxel_set_abstraction_spc import VoxelSetAbstractionSPC
    fix = sub(npz, "vsa_")
    mod = VoxelSetAbstractionSPC(to_attr(json.loads(str(npz["vsa_cfg"]))), VOXEL, PCR, num_bev_features=npz["vsa_bev"].shape[1],
                                 num_rawpoint_features=4)
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in sub(fix, "sd.").items()}, strict=True)
    mod = mod.cuda().eval()
    batch, _, _ = vsa_batch(npz, 'cuda')
    with torch.no_grad():
        whole = mod(dict(batch))['point_features_before_fusion'].clone()
        batch['rois'] = batch['rois'].clone()
        batch['rois'][1, :, 0:3] = 500.0
        bd = mod(dict(batch))
    n0 = int((fix["point_coords"][:, 0] == 0).sum())
    assert bd['point_coords'].shape[0] == n0 + 1
    first = int((npz["vsa_points"][:, 0] == 0).sum())
    assert np.array_equal(bd['point_coords'][-1].cpu().numpy(), npz["vsa_points"][first, :4])
    assert torch.allclose(bd['point_features_before_fusion'][:n0], whole[:n0], rtol=1e-5, atol=1e-6)
    pooled = bd['point_features_before_fusion'][-1, 16:]           # behind the 16 bev channels: raw_points, then x_conv2
    zero_in = {}
    for name, layer in (("x_conv2", mod.SA_layers[0]), ("raw_points", mod.SA_rawpoints)):
        outs = []
        for k in range(2):
            sub_layer = getattr(layer, "layer_%d" % k)
            width = sub_layer.separate_local_aggregation_layer[0].in_channels
            with torch.no_grad():
                outs.append(sub_layer.post_mlps(sub_layer.separate_local_aggregation_layer(torch.zeros((1, width, 1), device='cuda')))[0, :, 0])
        with torch.no_grad():
            zero_in[name] = layer.msg_post_mlps(torch.cat([bd['point_coords'][-1, 1:4]] + outs)[None, :, None])[0, :, 0]
    assert torch.allclose(pooled, torch.cat([zero_in["raw_points"], zero_in["x_conv2"]]), rtol=1e-5, atol=1e-6)


# ---- the point head and the RoI head over ragged keypoints ---------------------------------------------------------------------
@gpu
def test_gpu_ragged_point_head_against_the_reference(npz):
    """RaggedPointHeadSimple on 96 + 61 keypoints: the reference's labels exactly (a point in the enlarged box only, a point where
    only the other scene has a box, the classes of a three-class head), loss and tb_dict under the 4x rule."""
    from pdanet_amd.pv_rcnn_plusplus import RaggedPointHeadSimple
    fix = sub(npz, "point_")
    cfg = json.loads(str(fix["cfg"]))
    head = RaggedPointHeadSimple(num_class=1, input_channels=fix["features"].shape[1], model_cfg=to_attr(cfg))
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sub(fix, "sd.").items()}, strict=True)
    head = head.cuda().train()
    batch = {'batch_size': 2, 'point_features_before_fusion': dev(fix["features"]), 'point_features': None,
             'point_coords': dev(fix["coords"]), 'gt_boxes': dev(fix["gt_boxes"])}
    head(batch)
    assert np.array_equal(head.forward_ret_dict['point_cls_labels'].cpu().numpy(), fix["labels"])
    loss, tb = head.get_loss()
    check("point loss", rel(loss.detach().reshape(()), fix["loss_f64"]), rel(fix["loss"], fix["loss_f64"]))
    check("point tb point_loss_cls", rel(torch.as_tensor(tb['point_loss_cls']).detach().reshape(()), fix["tb_point_loss_cls_f64"]),
          rel(fix["tb_point_loss_cls"], fix["tb_point_loss_cls_f64"]))
    loss.backward()
    assert all(p.grad is not None for p in head.parameters())
    head3 = RaggedPointHeadSimple(num_class=3, input_channels=fix["features"].shape[1], model_cfg=to_attr(dict(cfg, CLASS_AGNOSTIC=False))).cuda()
    labels3 = head3.assign_targets({'point_coords': dev(fix["coords"]), 'gt_boxes': dev(fix["gt_boxes"])})['point_cls_labels']
    assert np.array_equal(labels3.cpu().numpy(), fix["labels_3"])


@gpu
def test_gpu_head_with_vector_pool_against_the_reference(npz):
    """PVRCNNPlusPlusHead, voxel_random_choice RoI-grid pool over 150 + 110 keypoints, train mode on the targets the reference
    sampled (handed over as roi_targets_dict): predictions, loss, every tb_dict entry and the keypoint-feature gradient."""
    from pdanet_amd.pv_rcnn_plusplus import PVRCNNPlusPlusHead
    fix = sub(npz, "head_")
    head = PVRCNNPlusPlusHead(input_channels=int(fix["c_in"]), model_cfg=to_attr(json.loads(str(fix["cfg"]))), num_class=1)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sub(fix, "sd.").items()}, strict=True)
    head = head.cuda().train()
    targets = {k: dev(v) for k, v in sub(fix, "target_").items()}
    f = dev(fix["point_features"]).requires_grad_(True)
    head({'batch_size': 2, 'rois': targets['rois'], 'roi_labels': targets['roi_labels'], 'roi_targets_dict': targets,
          'point_coords': dev(fix["point_coords"]), 'point_features': f, 'point_cls_scores': dev(fix["point_cls_scores"])})
    loss, tb = head.get_loss()
    loss.backward()
    for k in ("rcnn_cls", "rcnn_reg"):
        check("head " + k, rel(head.forward_ret_dict[k], fix[k + "_f64"]), rel(fix[k], fix[k + "_f64"]))
    check("head loss", rel(loss.detach().reshape(()), fix["loss_f64"]), rel(fix["loss"], fix["loss_f64"]))
    names = sorted(k[3:-4] for k in fix if k.startswith("tb_") and k.endswith("_f64"))
    assert sorted(tb) == names == ['rcnn_loss', 'rcnn_loss_cls', 'rcnn_loss_corner', 'rcnn_loss_reg']
    for k in names:
        check("head tb " + k, rel(torch.as_tensor(tb[k]).detach().reshape(()), fix["tb_" + k + "_f64"]), rel(fix["tb_" + k], fix["tb_" + k + "_f64"]))
    check("head d point_features", rel(f.grad, fix["grad_point_features_f64"]), rel(fix["grad_point_features"], fix["grad_point_features_f64"]))
    assert all(p.grad is not None for p in head.parameters())


# ---- the detector -------------------------------------------------------------------------------------------------------------
def reduced_detector_cfg():
    """pv_rcnn_plusplus.yaml's PFE, POINT_HEAD and ROI_HEAD on the reduced two-stage model of tests/golden/pv_rcnn_state_dict.json
    (32 x 32 x 40 cells of 0.05 x 0.05 x 0.1 m, a cut 2D backbone) with the Waymo yamls' first stage, CenterHead at
    FEATURE_MAP_STRIDE 8, as tests/test_centerpoint_voxel.py builds it; NUM_KEYPOINTS 128, 32 proposals, 16 sampled RoIs, a
    3 x 3 x 3 RoI grid, and raw points of one feature (NUM_REDUCED_CHANNELS 1)."""
    with open(os.path.join(HERE, "golden", "pv_rcnn_state_dict.json")) as f:
        model_cfg = json.load(f)['config']['MODEL']
    with open(os.path.join(HERE, "golden", "centerpoint_voxel_state_dict.json")) as f:
        kitti = json.load(f)['kitti']['config']
    head, ds = kitti['MODEL']['DENSE_HEAD'], kitti['dataset']
    head['TARGET_ASSIGNER_CONFIG']['FEATURE_MAP_STRIDE'] = 8
    head['POST_PROCESSING']['NMS_CONFIG']['NMS_POST_MAXSIZE'] = 32
    yaml_cfg = copy.deepcopy(FIXTURE['config']['pv_rcnn_plusplus'])
    model_cfg.update(NAME='PVRCNNPlusPlus', DENSE_HEAD=head, PFE=yaml_cfg['PFE'], POINT_HEAD=yaml_cfg['POINT_HEAD'], ROI_HEAD=yaml_cfg['ROI_HEAD'])
    model_cfg['PFE']['NUM_KEYPOINTS'] = 128
    model_cfg['PFE']['SA_LAYER']['raw_points']['NUM_REDUCED_CHANNELS'] = 1
    model_cfg['ROI_HEAD']['TARGET_CONFIG']['ROI_PER_IMAGE'] = 16
    model_cfg['ROI_HEAD']['ROI_GRID_POOL']['GRID_SIZE'] = 3
    return model_cfg, ds


@gpu
def test_gpu_pv_rcnn_plusplus_train_and_eval():
    """One training step and one eval forward on the reduced grid: a finite loss that is the sum of its parts, a gradient for
    every parameter, ragged keypoints.  The values of what this detector adds to the first stage -- point_loss_cls and the rcnn_*
    entries of tb_dict, and the keypoint encoder in front of them -- are compared with the reference under the 4x rule by the
    three tests above on fixed inputs; the first stage's rpn_loss by tests/test_centerpoint_voxel.py."""
    from pdanet_amd.pv_rcnn_plusplus import PVRCNNPlusPlus
    from pdanet_amd.voxel_utils import VoxelGenerator, collate_voxels
    model_cfg, ds = reduced_detector_cfg()
    B, counts = 2, [1500, 900]
    torch.manual_seed(3)
    model = PVRCNNPlusPlus(to_attr(model_cfg), 3, ds).cuda().train()
    rng = np.random.default_rng(5)
    pcr = np.array(ds['point_cloud_range'], np.float64)
    pts = np.concatenate([np.concatenate([rng.uniform(pcr[:3], pcr[3:], (n, 3)), rng.random((n, 1))], axis=1) for n in counts]).astype(np.float32)
    offs = torch.tensor([0, counts[0], sum(counts)], dtype=torch.int64).cuda()
    gen = VoxelGenerator(ds['voxel_size'], ds['point_cloud_range'], ds['num_point_features'], 5, 2000)
    voxels, coords, num_points = collate_voxels(*gen.generate_batch((dev(pts), offs, max(counts))))
    points = dev(np.concatenate([np.repeat(np.arange(B), counts)[:, None], pts], axis=1).astype(np.float32))
    gt = np.zeros((B, 3, 8), np.float32)                            # tests/test_centerpoint_voxel.py's boxes
    gt[0, 0] = [0.43, 0.03, -1.0, 0.45, 0.2, 0.17, 0.3, 1]
    gt[0, 1] = [1.13, 0.51, -0.6, 0.12, 0.1, 0.18, 1.2, 2]
    gt[0, 2] = [0.93, -0.47, -0.7, 0.2, 0.08, 0.17, -0.4, 3]
    gt[1, 0] = [0.71, -0.23, -0.6, 0.2, 0.09, 0.17, 2.0, 3]
    gt[1, 1] = [1.33, 0.31, -0.9, 0.4, 0.18, 0.16, -1.0, 1]
    batch = {'points': points, 'gt_boxes': dev(gt), 'batch_size': B, 'voxels': voxels, 'voxel_coords': coords, 'voxel_num_points': num_points}
    ret, tb, disp = model(dict(batch, roi_target_seed=11))
    assert torch.isfinite(ret['loss']) and disp == {}
    assert set(tb) == {'hm_loss_head_0', 'loc_loss_head_0', 'rpn_loss', 'point_loss_cls', 'point_pos_num', 'rcnn_loss_cls',
                       'rcnn_loss_reg', 'rcnn_loss_corner', 'rcnn_loss'}
    assert float(ret['loss'].detach()) == pytest.approx(float(tb['rpn_loss'] + tb['point_loss_cls'] + tb['rcnn_loss']), rel=1e-5)
    assert model.roi_head.forward_ret_dict['rcnn_cls'].shape == (B * 16, 1)
    n_key = model.point_head.forward_ret_dict['point_cls_labels'].shape[0]
    assert 2 <= n_key <= B * (128 + 6)                               # ragged: every sector's quota rounds up
    ret['loss'].backward()
    for name, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    model.eval()
    with torch.no_grad():
        pred_dicts, recall = model(dict(batch))
    assert len(pred_dicts) == B and set(pred_dicts[0]) == {'pred_boxes', 'pred_scores', 'pred_labels'}
    assert set(recall) == {'gt', 'roi_0.3', 'rcnn_0.3', 'roi_0.5', 'rcnn_0.5', 'roi_0.7', 'rcnn_0.7'}
