"""CaDDN: the fused frustum-to-voxel sampling and the one-pass DDNLoss (csrc/frustum_sample.hip), ImageVFE, DDNDeepLabV3,
Conv2DCollapse and the detector, against the reference's own CPU run (tests/golden/caddn.npz, made by make_caddn_golden.py)
and a float64 numpy restatement of the factorised formula (tests/golden/frustum_sample_restatement.py).

Tolerances follow test_second_iou.py.  The bound for a device result is computed here, never from the kernel: FACTOR = 4 times
the largest error of torch's own float32 CPU composition (image_vfe.frustum_to_voxel_composed, ddn_loss_composed, or their
autograd) against the float64 truth on the same inputs, plus 2^-23 x max |truth| -- both are float32 evaluations of one
formula that differ in operation order.  The whole model follows test_voxel_rcnn.py: the fixture holds the reference's
float32 CPU run and its float64 run; the device may be off from the float64 run by FACTOR times what the float32 run is off,
one figure over all loss terms (normalised by the largest) and one over the recorded gradients, plus 2^-23.  Every figure is
printed."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from pdanet_amd.config import to_attr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import frustum_sample_restatement as rs  # noqa: E402

gpu = pytest.mark.gpu
FACTOR = 4.0
EPS32 = 2.0 ** -23
with open(os.path.join(HERE, "golden", "caddn_state_dict.json")) as _f:
    FIXTURE = json.load(_f)
CFG = FIXTURE['config']
DISC = {"mode": "LID", "num_bins": 8, "depth_min": 2.0, "depth_max": 14.0}
SHAPES = [[27, 43], [25, 41]]
GRIDS = {'wide': ([12, 16, 5], [2.0, -8.0, -3.0, 14.0, 8.0, 2.0]),            # the fixture's
         'long': ([70, 3, 2], [2.0, -1.5, -1.0, 14.0, 1.5, 1.0])}             # X crosses a wave boundary
LOSS_ARGS = {"weight": 3.0, "alpha": 0.25, "gamma": 2.0, "fg_weight": 13.0, "bg_weight": 1.0}


@pytest.fixture(scope="module")
def npz():
    with np.load(os.path.join(HERE, "golden", "caddn.npz")) as f:
        return {k: f[k] for k in f.files}


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def composed(feat, logits, l2c, c2i, grid, pcr, disc, dtype, grad_out=None):
    """image_vfe.frustum_to_voxel_composed on the CPU in `dtype`: the output, and with grad_out the gradients of feat and
    depth_logits."""
    from pdanet_amd.image_vfe import frustum_to_voxel_composed
    f, x = t32(feat).to(dtype).requires_grad_(grad_out is not None), t32(logits).to(dtype).requires_grad_(grad_out is not None)
    out = frustum_to_voxel_composed(f, x, t32(l2c).to(dtype), t32(c2i).to(dtype), torch.tensor(SHAPES, dtype=torch.int32), grid, pcr, disc)
    if grad_out is None:
        return out.detach().numpy()
    out.backward(t32(grad_out).to(dtype))
    return out.detach().numpy(), f.grad.numpy(), x.grad.numpy()


def fused(feat, logits, l2c, c2i, grid, pcr, disc, grad_out=None):
    """FrustumToVoxel's fused path on the device: softmax in torch, pda_frustum_sample_fwd / _bwd."""
    from pdanet_amd.image_vfe import FrustumToVoxel
    mod = FrustumToVoxel(to_attr({"SAMPLER": {"mode": "bilinear", "padding_mode": "zeros"}}), grid, pcr, disc)
    f, x = t32(feat).cuda().requires_grad_(grad_out is not None), t32(logits).cuda().requires_grad_(grad_out is not None)
    out = mod({"image_features": f, "depth_logits": x, "trans_lidar_to_cam": t32(l2c).cuda(), "trans_cam_to_img": t32(c2i).cuda(),
               "image_shape": torch.tensor(SHAPES, dtype=torch.int32).cuda()})["voxel_features"]
    if grad_out is None:
        return out.detach().cpu().numpy()
    out.backward(t32(grad_out).cuda())
    return out.detach().cpu().numpy(), f.grad.cpu().numpy(), x.grad.cpu().numpy()


def prob64(logits):
    return torch.softmax(t32(logits).double(), 1)[:, :-1].numpy()


class Case:
    """One sampling case with its float64 truths and the bounds, computed once."""

    def __init__(self, name, feat, logits, l2c, c2i, grid, pcr, disc, seed=1):
        self.name, self.args = name, (feat, logits, l2c, c2i, grid, pcr, disc)
        self.truth, self.inside = rs.frustum_sample(feat, prob64(logits), l2c, c2i, np.asarray(SHAPES), grid, pcr, disc)
        self.grad_out = np.random.default_rng(seed).standard_normal(self.truth.shape).astype(np.float32)
        out64, self.df, self.dx = composed(*self.args, torch.float64, self.grad_out)
        assert np.abs(out64 - self.truth).max() <= 1e-12 * max(np.abs(self.truth).max(), 1.0)    # the identity of the factorisation
        out32, df32, dx32 = composed(*self.args, torch.float32, self.grad_out)
        self.e_torch = [float(np.abs(a - b).max()) for a, b in ((out32, self.truth), (df32, self.df), (dx32, self.dx))]
        self.bound = [FACTOR * e + EPS32 * float(np.abs(t).max()) for e, t in zip(self.e_torch, (self.truth, self.df, self.dx))]
        self.share = self.inside.reshape(len(feat), -1).mean(1)


def draw(rng, C, Hf=7, Wf=11, nb=8):
    return (rng.standard_normal((2, C, Hf, Wf)).astype(np.float32), rng.standard_normal((2, nb + 1, Hf, Wf)).astype(np.float32))


@pytest.fixture(scope="module")
def cases(npz):
    """C in {5, 64, 70} on the fixture's grid (C = 5 is the fixture itself) and on the long one; UD and SID; the hostile ones."""
    rng = np.random.default_rng(64)
    l2c, c2i = npz["f2v_l2c"], npz["f2v_c2i"]
    out = {}
    for gname, (grid, pcr) in GRIDS.items():
        for C in (5, 64, 70):
            feat, logits = (npz["f2v_feat"], npz["f2v_logits"]) if (gname, C) == ('wide', 5) else draw(rng, C)
            out["%s-%d" % (gname, C)] = Case("%s-%d" % (gname, C), feat, logits, l2c, c2i, grid, pcr, DISC)
    for mode in ("UD", "SID"):
        out[mode] = Case(mode, *draw(rng, 6), l2c, c2i, *GRIDS['wide'], dict(DISC, mode=mode))
    grid, pcr = GRIDS['wide']
    near = l2c.copy()
    near[:, 2, 3] -= 3.0                                                       # the camera moved forward: depths below depth_min
    out["hostile-near"] = Case("hostile-near", *draw(rng, 6), near, c2i, grid, pcr, DISC)
    bad_l, bad_c = l2c.copy(), c2i.copy()
    bad_l[0, 1, 2], bad_c[1, 0, 0] = np.nan, np.inf
    out["hostile-nonfinite"] = Case("hostile-nonfinite", *draw(rng, 6), bad_l, bad_c, grid, pcr, DISC)
    flat_l, flat_c = l2c.copy(), c2i.copy()
    flat_l[0] = np.array([[0, -1, 0, 0.1], [0, 0, -1, 0.2], [1, 0, 0, -2.5], [0, 0, 0, 1]], np.float32)   # voxel i = 0: cam z = 0 exactly
    flat_c[0, 2, 3] = 0.0
    out["hostile-zero-depth"] = Case("hostile-zero-depth", *draw(rng, 6), flat_l, flat_c, grid, pcr, DISC)
    return out


REGULAR = ["%s-%d" % (g, c) for g in GRIDS for c in (5, 64, 70)]
HOSTILE = ["hostile-near", "hostile-nonfinite", "hostile-zero-depth"]


# ---- without a GPU --------------------------------------------------------------------------------------------------------
def build_yaml_model():
    from pdanet_amd.caddn import CaDDN
    return CaDDN(to_attr(FIXTURE['yaml']['MODEL']), 3, FIXTURE['yaml']['dataset'])


def test_state_dict_layout_is_the_references():
    before = json.dumps(FIXTURE['yaml']['MODEL'], sort_keys=True)
    model = build_yaml_model()
    own = model.state_dict()
    assert [[k, list(v.shape)] for k, v in own.items()] == FIXTURE['CaDDN']
    for key, shape in (("vfe.ffn.ddn.model.backbone.layer1.0.downsample.0.weight", [256, 64, 1, 1]),
                       ("vfe.ffn.ddn.model.backbone.layer3.5.conv2.weight", [256, 256, 3, 3]),
                       ("vfe.ffn.ddn.model.classifier.0.convs.4.1.weight", [256, 2048, 1, 1]),
                       ("vfe.ffn.ddn.model.classifier.0.project.0.weight", [256, 1280, 1, 1]),
                       ("vfe.ffn.ddn.model.classifier.4.bias", [81]), ("vfe.ffn.channel_reduce.conv.weight", [64, 256, 1, 1]),
                       ("map_to_bev_module.block.conv.weight", [64, 1600, 1, 1])):
        assert list(own[key].shape) == shape, key
    # torchvision's deeplabv3_resnet50 without the aux classifier: 53 + 7 + 2 convolutions and 60 BatchNorms of five entries
    ddn = [k for k in own if k.startswith("vfe.ffn.ddn.model.")]
    assert len(ddn) == 362 and not any("aux_classifier" in k for k in own)
    assert [n for n, _ in model.named_children()] == ['vfe', 'map_to_bev_module', 'backbone_2d', 'dense_head']
    assert [n for n, _ in model.vfe.named_children()] == ['ffn', 'f2v']
    assert [n for n, _ in model.vfe.ffn.named_children()][:2] == ['ddn', 'channel_reduce']
    # layer3 and layer4 are dilated, not strided; the stride of layer2 sits on conv2
    bb = model.vfe.ffn.ddn.model.backbone
    assert bb['layer2'][0].conv2.stride == (2, 2) and bb['layer2'][0].conv1.stride == (1, 1)
    assert bb['layer3'][0].conv2.stride == (1, 1) and bb['layer3'][0].conv2.dilation == (1, 1) and bb['layer3'][1].conv2.dilation == (2, 2)
    assert bb['layer4'][0].conv2.dilation == (2, 2) and bb['layer4'][2].conv2.dilation == (4, 4)
    assert [c[0].dilation for c in model.vfe.ffn.ddn.model.classifier[0].convs[1:4]] == [(12, 12), (24, 24), (36, 36)]
    # the anchors lie on the feature_map_stride 2 grid
    assert all(tuple(a.shape[:3]) == (1, 188, 140) for a in model.dense_head.anchors)
    assert json.dumps(FIXTURE['yaml']['MODEL'], sort_keys=True) == before                 # the config is not modified
    sd = {k: torch.zeros(shape, dtype=own[k].dtype) for k, shape in FIXTURE['CaDDN']}
    model.load_state_dict(sd, strict=True)


def test_build_and_refusals():
    from pdanet_amd import caddn
    cfg = json.loads(json.dumps(FIXTURE['yaml']['MODEL']))
    cfg['NAME'] = 'PointPillar'
    with pytest.raises(NotImplementedError, match="PointPillar"):
        caddn.build(to_attr(cfg), 3, FIXTURE['yaml']['dataset'])
    cfg = json.loads(json.dumps(FIXTURE['yaml']['MODEL']))
    cfg['VFE']['FFN']['DISCRETIZE']['mode'] = 'XID'
    with pytest.raises(NotImplementedError, match="XID"):
        caddn.build(to_attr(cfg), 3, FIXTURE['yaml']['dataset'])
    ds = {k: v for k, v in FIXTURE['yaml']['dataset'].items() if k != 'depth_downsample_factor'}
    with pytest.raises(ValueError, match="depth_downsample_factor"):
        caddn.depth_downsample_factor(ds)
    ds['DATA_PROCESSOR'] = [{'NAME': 'calculate_grid_size', 'VOXEL_SIZE': [0.16] * 3}, {'NAME': 'downsample_depth_map', 'DOWNSAMPLE_FACTOR': 4}]
    assert caddn.depth_downsample_factor(ds) == 4


def test_ddn_deeplabv3_shapes_and_missing_checkpoint(tmp_path, monkeypatch):
    from pdanet_amd.ddn_deeplabv3 import DDNDeepLabV3
    net = DDNDeepLabV3(backbone_name='ResNet50', feat_extract_layer='layer1', num_classes=9).eval()
    images = torch.rand(2, 3, 32, 48)
    with torch.no_grad():
        res = net(images)
    assert tuple(res['features'].shape) == (2, 256, 8, 12) and tuple(res['logits'].shape) == (2, 9, 8, 12)
    assert torch.isfinite(res['logits']).all()
    # a missing checkpoint raises, and nothing reaches for the network
    import urllib.request
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", lambda *a, **k: pytest.fail("download"))
    monkeypatch.setattr(urllib.request, "urlopen", lambda *a, **k: pytest.fail("download"))
    missing = str(tmp_path / "checkpoints" / "deeplabv3_resnet50_coco.pth")
    with pytest.raises(FileNotFoundError, match="deeplabv3_resnet50_coco"):
        DDNDeepLabV3(backbone_name='ResNet50', feat_extract_layer='layer1', num_classes=9, pretrained_path=missing)
    assert not os.path.exists(os.path.dirname(missing))
    # a checkpoint with 21 classes and an aux classifier loads through filter_pretrained_dict; preprocess then runs
    sd = {k: torch.full_like(v, 0.5) for k, v in net.model.state_dict().items()}
    sd["classifier.4.weight"], sd["classifier.4.bias"] = torch.zeros(21, 256, 1, 1), torch.zeros(21)
    sd["aux_classifier.0.weight"] = torch.zeros(256, 1024, 3, 3)
    path = str(tmp_path / "ckpt.pth")
    torch.save(sd, path)
    loaded = DDNDeepLabV3(backbone_name='ResNet50', feat_extract_layer='layer1', num_classes=9, pretrained_path=path)
    assert float(loaded.model.backbone['conv1'].weight[0, 0, 0, 0]) == 0.5 and tuple(loaded.model.classifier[4].weight.shape) == (9, 256, 1, 1)
    images[0, :, 30:, :] = float('nan')
    x = loaded.preprocess(images)
    assert torch.isfinite(x).all() and not x[0, :, 30:, :].any()
    assert torch.allclose(x[1, 0], (images[1, 0] - 0.485) / 0.229)


def test_symbols_exist_and_sizes_are_checked_before_any_launch():
    from pdanet_amd import build, _lib
    build.build()
    lib = _lib.load()
    for name in ("pda_frustum_sample_fwd", "pda_frustum_sample_bwd", "pda_ddn_loss_fwd_bwd", "pda_ddn_loss_blocks"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.pda_abi_version() == 20
    f, f3 = ctypes.c_float, (ctypes.c_float * 3)(1, 1, 1)
    fwd = lambda b, c, d, hf, wf, gx, gy, gz, mode=1, lo=2.0, hi=46.8, geo=f3: lib.pda_frustum_sample_fwd(   # noqa: E731
        None, None, None, None, None, None, b, c, d, hf, wf, gx, gy, gz, geo, geo, mode, f(lo), f(hi), None)
    bwd = lambda b, c, d, hf, wf, gx, gy, gz, mode=1, lo=2.0, hi=46.8, geo=f3: lib.pda_frustum_sample_bwd(   # noqa: E731
        None, None, None, None, None, None, None, None, b, c, d, hf, wf, gx, gy, gz, geo, geo, mode, f(lo), f(hi), None)
    for entry in (fwd, bwd):
        assert entry(0, 64, 80, 94, 311, 280, 376, 25) == 0                                    # empty: returns at once
        for bad, word in (((-1, 64, 80, 94, 311, 280, 376, 25), b"batch"), ((65536, 64, 80, 94, 311, 280, 376, 25), b"batch"),
                          ((2, 0, 80, 94, 311, 280, 376, 25), b"channels"), ((2, 64, 1, 94, 311, 280, 376, 25), b"bins"),
                          ((2, 64, 80, 0, 311, 280, 376, 25), b"feature map"), ((2, 64, 80, 94, 1 << 30, 280, 376, 25), b"feature map"),
                          ((2, 64, 80, 94, 311, 0, 376, 25), b"grid"), ((2, 64, 80, 94, 311, 280, 376, -1), b"grid")):
            assert entry(*bad) == 1 and word in lib.pda_last_error(), bad
        assert entry(2, 64, 80, 94, 311, 280, 376, 25, mode=3) == 1 and b"mode" in lib.pda_last_error()
        assert entry(2, 64, 80, 94, 311, 280, 376, 25, lo=5.0, hi=5.0) == 1 and b"depth range" in lib.pda_last_error()
        assert entry(2, 64, 80, 94, 311, 280, 376, 25, geo=None) == 1 and b"null" in lib.pda_last_error()
        assert entry(2, 64, 80, 94, 311, 280, 376, 25) == 1 and b"null" in lib.pda_last_error()
    d = ctypes.c_double
    loss = lambda b, nb, h, w, n, mode=1, lo=2.0, hi=46.8, ds=4.0: lib.pda_ddn_loss_fwd_bwd(                 # noqa: E731
        None, None, None, None, None, None, b, nb, h, w, n, mode, f(lo), f(hi), f(ds), d(0.25), d(2), d(13), d(1), d(3), None)
    for bad, word in (((0, 80, 94, 311, 5), b"batch"), ((2, 80, 0, 311, 5), b"map"), ((2, 0, 94, 311, 5), b"bins"),
                      ((2, 80, 94, 311, -1), b"boxes")):
        assert loss(*bad) == 1 and word in lib.pda_last_error(), bad
    assert loss(2, 80, 94, 311, 5, mode=-1) == 1 and b"mode" in lib.pda_last_error()
    assert loss(2, 80, 94, 311, 5, ds=0.0) == 1 and b"downsample" in lib.pda_last_error()
    assert loss(2, 80, 94, 311, 5) == 1 and b"null" in lib.pda_last_error()
    assert lib.pda_ddn_loss_blocks(0) == 0 and lib.pda_ddn_loss_blocks(257) == 2 and lib.pda_ddn_loss_blocks(1 << 30) == 1024


def test_composed_path_reproduces_the_reference_run(npz, cases):
    """On the CPU: the torch composition, the restatement and the reference's recorded float32 run agree."""
    from pdanet_amd import image_vfe as iv
    from pdanet_amd.conv2d_collapse import Conv2DCollapse
    grid, pcr = GRIDS['wide']
    frustum = iv.create_frustum_features(t32(npz["f2v_feat"]), t32(npz["f2v_logits"])).numpy()
    assert frustum.shape == (2, 5, 8, 7, 11) and np.abs(frustum - npz["f2v_frustum"]).max() <= 2 * EPS32 * np.abs(frustum).max()
    case = cases['wide-5']
    out = composed(npz["f2v_feat"], npz["f2v_logits"], npz["f2v_l2c"], npz["f2v_c2i"], grid, pcr, DISC, torch.float32)
    e_ref, e_own = float(np.abs(npz["f2v_out"] - case.truth).max()), float(np.abs(out - case.truth).max())
    print("f2v: reference in float32 against the float64 restatement %.3e, this torch on the CPU %.3e, max |out| %.3f"
          % (e_ref, e_own, float(np.abs(case.truth).max())))
    # positions carry a few float32 roundings of pixel coordinates up to 43; features of unit size
    assert npz["f2v_out"].shape == (2, 5, 5, 16, 12) and e_ref < 2e-5 and e_own < 2e-5
    # every scene keeps voxels inside and outside the frustum, in every case but the hostile ones
    for name, c in cases.items():
        print(name, "share of voxels inside", c.share, "torch float32 errors", c.e_torch)
        if not name.startswith("hostile"):
            assert np.all((c.share >= 0.2) & (c.share <= 0.9)), name
        assert not c.truth.transpose(0, 2, 3, 4, 1)[~c.inside].any() and np.isfinite(c.truth).all() and np.isfinite(c.dx).all()
    assert cases["hostile-nonfinite"].share.max() == 0 and 0 < cases["hostile-near"].share.min()
    assert not cases["hostile-zero-depth"].inside[0, :, :, 0].any() and cases["hostile-zero-depth"].inside[0].any()
    # DDNLoss
    want = rs.ddn_loss(npz["ddn_logits"], npz["ddn_depth"], npz["ddn_boxes"], DISC, 4.0, **LOSS_ARGS)
    x = t32(npz["ddn_logits"]).requires_grad_()
    boxes = t32(npz["ddn_boxes"].copy())
    mod = iv.DDNLoss(disc_cfg=DISC, downsample_factor=4, **LOSS_ARGS)
    os.environ[iv.ENV_LOSS] = "composed"
    try:
        loss, tb = mod(x, t32(npz["ddn_depth"]), boxes)
    finally:
        del os.environ[iv.ENV_LOSS]
    loss.backward()
    assert set(tb) == {"balancer_loss", "fg_loss", "bg_loss", "ddn_loss"} and all(v.dim() == 0 and not v.requires_grad for v in tb.values())
    assert np.array_equal(boxes.numpy(), npz["ddn_boxes"])
    got = np.array([float(loss), float(tb["fg_loss"]), float(tb["bg_loss"]), float(tb["balancer_loss"])])
    ref = np.array([want[0], want[1], want[2], want[1] + want[2]])
    print("ddn: composed", got, "reference", npz["ddn_loss"], "restatement", ref)
    assert np.abs(got - ref).max() < 1e-5 * ref[0] and np.abs(npz["ddn_loss"] - ref).max() < 1e-5 * ref[0]
    assert np.abs(x.grad.numpy() - want[3]).max() < 1e-6 and np.abs(npz["ddn_grad"] - want[3]).max() < 1e-6
    assert want[5].any() and not want[5].all() and (want[4] == 8).sum() > 20 and len(np.unique(want[4])) == 9
    # Conv2DCollapse
    col = Conv2DCollapse(to_attr({"NUM_BEV_FEATURES": 5, "ARGS": {"kernel_size": 1, "stride": 1, "bias": False}}), grid)
    col.load_state_dict({k[len("col_sd."):]: t32(v) for k, v in npz.items() if k.startswith("col_sd.")}, strict=True)
    col.eval()
    with torch.no_grad():
        bev = col({"voxel_features": t32(npz["f2v_out"])})["spatial_features"].numpy()
    assert bev.shape == (2, 5, 16, 12) and np.abs(bev - npz["col_out"]).max() <= 1e-5 * np.abs(npz["col_out"]).max()


# ---- on the GPU -------------------------------------------------------------------------------------------------------------
def report(case, what, got, truth, k):
    e = float(np.abs(got - truth).max())
    print("%s %s: device %.3e, torch in float32 on the CPU %.3e, bound %.3e, max |truth| %.3f"
          % (case.name, what, e, case.e_torch[k], case.bound[k], float(np.abs(truth).max())))
    return e


@gpu
@pytest.mark.parametrize("name", REGULAR + ["UD", "SID"])
def test_fused_forward_equals_the_restatement(cases, name):
    case = cases[name]
    out = fused(*case.args)
    assert out.shape == case.truth.shape
    e = report(case, "forward", out, case.truth, 0)
    assert e <= case.bound[0]
    assert not out.transpose(0, 2, 3, 4, 1)[~case.inside].any()                    # outside the frustum: exact zeros


@gpu
@pytest.mark.parametrize("name", REGULAR)
def test_fused_backward_equals_float64_autograd(cases, name):
    case = cases[name]
    _, df, dx = fused(*case.args, grad_out=case.grad_out)
    e_f, e_x = report(case, "d features", df, case.df, 1), report(case, "d depth_logits", dx, case.dx, 2)
    assert e_f <= case.bound[1] and e_x <= case.bound[2]


@gpu
@pytest.mark.parametrize("name", HOSTILE)
def test_hostile_geometry(cases, name):
    case = cases[name]
    out, df, dx = fused(*case.args, grad_out=case.grad_out)
    e = report(case, "forward", out, case.truth, 0)
    e_f, e_x = report(case, "d features", df, case.df, 1), report(case, "d depth_logits", dx, case.dx, 2)
    assert e <= case.bound[0] and e_f <= case.bound[1] and e_x <= case.bound[2]
    assert not out.transpose(0, 2, 3, 4, 1)[~case.inside].any()
    assert np.isfinite(out).all() and np.isfinite(df).all() and np.isfinite(dx).all()


@gpu
def test_ddn_loss_equals_the_restatement(npz):
    from pdanet_amd import image_vfe as iv
    want = rs.ddn_loss(npz["ddn_logits"], npz["ddn_depth"], npz["ddn_boxes"], DISC, 4.0, **LOSS_ARGS)
    truth = np.array([want[0], want[1], want[2]])
    x32 = t32(npz["ddn_logits"]).requires_grad_()
    cpu = iv.ddn_loss_composed(x32, t32(npz["ddn_depth"]), t32(npz["ddn_boxes"]), DISC, 4.0, **LOSS_ARGS)
    cpu[0].backward()
    e_torch = np.abs(np.array([float(v) for v in cpu]) - truth)
    e_grad_torch = float(np.abs(x32.grad.numpy() - want[3]).max())
    mod = iv.DDNLoss(disc_cfg=DISC, downsample_factor=4, **LOSS_ARGS)
    x, boxes = t32(npz["ddn_logits"]).cuda().requires_grad_(), t32(npz["ddn_boxes"]).cuda()
    depth = t32(npz["ddn_depth"]).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, tb = mod(x, depth, boxes)
        (loss * 2.0).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(v.dim() == 0 and v.is_cuda for v in list(tb.values()) + [loss])
    assert np.array_equal(boxes.cpu().numpy().view(np.uint32), npz["ddn_boxes"].view(np.uint32))       # bitwise unchanged
    got = np.array([float(loss), float(tb["fg_loss"]), float(tb["bg_loss"])])
    bound = FACTOR * e_torch + EPS32 * np.abs(truth)
    print("ddn loss, fg, bg: device off by", np.abs(got - truth), "torch in float32 on the CPU", e_torch, "bound", bound)
    assert np.all(np.abs(got - truth) <= bound)
    assert abs(float(tb["balancer_loss"]) - (want[1] + want[2])) <= bound[1] + bound[2] and float(tb["ddn_loss"]) == float(loss)
    e_grad = float(np.abs(x.grad.cpu().numpy() / 2.0 - want[3]).max())
    g_bound = FACTOR * e_grad_torch + EPS32 * float(np.abs(want[3]).max())
    print("ddn d logits: device %.3e, torch in float32 on the CPU %.3e, bound %.3e" % (e_grad, e_grad_torch, g_bound))
    assert e_grad <= g_bound


def err_dict(got, ref):
    """one figure over a dict of arrays, normalised by the largest reference entry"""
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    scale = max(float(np.abs(np.asarray(r, np.float64)).max()) for r in ref.values())
    return max(float(np.abs(np.asarray(got[k], np.float64) - np.asarray(ref[k], np.float64)).max()) for k in ref) / scale


def fixture_model(npz, monkeypatch):
    from pdanet_amd import image_vfe as iv
    from pdanet_amd.caddn import build
    monkeypatch.setattr(iv.DepthFFN, "DDN", {"DDNDeepLabV3": rs.TwoConvDDN})
    model = build(to_attr(json.loads(json.dumps(CFG['MODEL']))), 3, CFG['dataset'])
    model.load_state_dict({k[len("net_sd."):]: t32(v) for k, v in npz.items() if k.startswith("net_sd.")}, strict=True)
    return model


def fixture_batch(npz, device):
    bd = {k[len("net_in."):]: t32(v).to(device) for k, v in npz.items() if k.startswith("net_in.")}
    bd["batch_size"] = 2
    return bd


def test_fixture_model_loads_the_reference_parameters(npz, monkeypatch):
    model = fixture_model(npz, monkeypatch)
    assert [n for n, _ in model.named_children()] == ['vfe', 'map_to_bev_module', 'backbone_2d', 'dense_head']
    assert all(tuple(a.shape[:3]) == (1, 8, 6) for a in model.dense_head.anchors)       # grid 12 x 16 at feature_map_stride 2
    assert np.isnan(npz["net_in.images"]).any() and np.isnan(npz["net_in.depth_maps"]).any()


@gpu
def test_model_training_forward_and_eval(npz, monkeypatch):
    model = fixture_model(npz, monkeypatch).cuda()
    model.eval()
    with torch.no_grad():
        preds, recall = model(fixture_batch(npz, "cuda"))
    for b, p in enumerate(preds):
        labels, scores = npz["net_eval%d.pred_labels" % b], npz["net_eval%d.pred_scores" % b]
        print("scene %d: labels %s scores %s (reference %s)" % (b, p["pred_labels"].tolist(), p["pred_scores"].tolist(), scores.tolist()))
        assert len(p["pred_scores"]) == len(scores) >= 2
        assert p["pred_labels"].cpu().numpy().tolist() == labels.tolist()               # count, labels and order
        assert np.abs(p["pred_scores"].cpu().numpy() - scores).max() < 1e-4
        assert np.abs(p["pred_boxes"].cpu().numpy() - npz["net_eval%d.pred_boxes" % b]).max() < 1e-3
    model.train()
    stats = {k: v.clone() for k, v in model.state_dict().items()}
    model(fixture_batch(npz, "cuda"))[0]['loss'].backward()                              # warm-up: lazy initialisation may read
    model.load_state_dict(stats)
    model.zero_grad()
    bd = fixture_batch(npz, "cuda")
    boxes2d = bd["gt_boxes2d"].clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                              # forward + loss + backward: no host read
    try:
        ret, tb, disp = model(bd)
        ret['loss'].backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(bd["gt_boxes2d"], boxes2d)
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 and v.is_cuda for v in tb.values())
    names = [str(n) for n in npz["net_term_names"]]
    got = dict({k: float(v) for k, v in tb.items()}, loss=float(ret['loss']))
    gold, truth = dict(zip(names, npz["net_terms"])), dict(zip(names, npz["net_terms_f64"]))
    e_dev, e_gold = err_dict(got, truth), err_dict(gold, truth)
    print("loss terms: device %.3e, reference in float32 on the CPU %.3e" % (e_dev, e_gold), got)
    assert e_dev <= FACTOR * e_gold + EPS32
    params = dict(model.named_parameters())
    keys = [k[len("net_grad_f64."):] for k in npz if k.startswith("net_grad_f64.")]
    assert len(keys) == 6
    g_dev = {k: params[k].grad.cpu().numpy() for k in keys}
    g_gold, g_truth = {k: npz["net_grad." + k] for k in keys}, {k: npz["net_grad_f64." + k] for k in keys}
    e_dev, e_gold = err_dict(g_dev, g_truth), err_dict(g_gold, g_truth)
    print("gradients: device %.3e, reference in float32 on the CPU %.3e" % (e_dev, e_gold))
    assert e_dev <= FACTOR * e_gold + EPS32


@gpu
def test_the_frustum_tensor_is_gone():
    """At C = 64, D = 80, feature map 24 x 78, grid 70 x 94 x 25: the fused forward + backward stays within the inputs, the
    output and their gradients plus 10 %; the composition needs at least the frustum tensor more."""
    from pdanet_amd import image_vfe as iv
    B, C, D, Hf, Wf, grid = 1, 64, 80, 24, 78, [70, 94, 25]
    pcr = [2, -30.08, -3.0, 46.8, 30.08, 1.0]
    disc = dict(mode="LID", num_bins=D, depth_min=2.0, depth_max=46.8)
    l2c, c2i = rs.calibration(np.random.default_rng(3), [(96, 312)], focal=180.0)
    geo = (t32(l2c).cuda(), t32(c2i).cuda(), torch.tensor([[96, 312]], dtype=torch.int32).cuda(), grid, pcr, disc)
    g = torch.Generator(device="cuda").manual_seed(1)

    def peak(run):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        feat = torch.randn(B, C, Hf, Wf, device="cuda", generator=g).requires_grad_()
        out = run(feat)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out            # read before anything is computed from the output

    def run_fused(feat):
        prob = torch.softmax(torch.randn(B, D + 1, Hf, Wf, device="cuda", generator=g), 1)[:, :-1].contiguous().requires_grad_()
        out = iv.frustum_sample(feat, prob, *geo)
        out.backward(torch.ones_like(out))
        assert feat.grad is not None and prob.grad is not None
        return out.detach()

    def run_composed(feat):
        logits = torch.randn(B, D + 1, Hf, Wf, device="cuda", generator=g).requires_grad_()
        out = iv.frustum_to_voxel_composed(feat, logits, *geo)
        out.backward(torch.ones_like(out))
        return None

    run_fused(torch.randn(B, C, Hf, Wf, device="cuda", generator=g).requires_grad_())         # warm-up
    fused_peak, out = peak(run_fused)
    nonzero = float((out != 0).float().mean())
    del out
    composed_peak, _ = peak(run_composed)
    voxels = B * C * grid[0] * grid[1] * grid[2] * 4
    needed = 2 * (voxels + B * (C + D) * Hf * Wf * 4)
    frustum = B * C * D * Hf * Wf * 4
    print("peak memory: fused %.1f MB (inputs, output and gradients %.1f MB), composed %.1f MB, frustum tensor %.1f MB, non-zero "
          "voxels %.2f" % (fused_peak / 1e6, needed / 1e6, composed_peak / 1e6, frustum / 1e6, nonzero))
    assert 0.2 < nonzero < 0.9
    assert fused_peak <= 1.1 * needed
    assert composed_peak >= fused_peak + frustum
