"""PointRCNN: the canonical RoI point pool (csrc/roi_pool.hip, pda_roipoint_pool3d_canonical_fwd), PointnetSAModuleMSG /
PointnetSAModule, PointNet2MSG, PointResidualCoder, PointHeadBox, PointRCNNHead and PointRCNN against the reference's own CPU
runs in float32 and float64 (tests/golden/pointrcnn.npz, made by make_pointrcnn_golden.py) and, for the kernel, against the
reference's composition over RoIPointPool3d on the same device.

Tolerances.  Kernel: the selection, the copied columns (score, features) and the flag are bit-equal to the composed path; the
canonical xyz is bit-equal where the heading is 0 and the coordinates lie on the 1/8 lattice, elsewhere within 1e-5 for RoIs
under 10 m (two float32 cos / sin results of <= 2 ulp each on offsets of a few metres); the depth column within 1e-6 (a
float32 sqrt of a three-term sum is <= 2 ulp, then scaled by 1/70).  Modules: for a tensor, e = max |ref32 - ref64| relative
to the tensor's largest magnitude; the device passes when it is within FACTOR x e of the float64 values -- its own rounding
is of the size of the reference's, and a different sum order and fma contraction may double it once more -- and within FLOOR
where e = 0 because the values are exact (a gradient that is zero in exact arithmetic is one such: check_grads).  Discrete
outputs (FPS picks, labels, the zero pattern of the box labels) are exact.  Every figure is printed."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from pdanet_amd.config import to_attr

HERE = os.path.dirname(os.path.abspath(__file__))
gpu = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 1e-6
XYZ_TOL, DEPTH_TOL = 1e-5, 1e-6
with open(os.path.join(HERE, "golden", "pointrcnn_state_dict.json")) as _f:
    FIXTURE = json.load(_f)
CFG = FIXTURE['config']
SYMBOL = "pda_roipoint_pool3d_canonical_fwd"
MISSES = []                      # (what, deviation, bound) of the checks that missed since the last settle()


@pytest.fixture(scope="module")
def npz():
    with np.load(os.path.join(HERE, "golden", "pointrcnn.npz")) as f:
        return {k: f[k] for k in f.files}


def sub(npz, prefix):
    return {k[len(prefix):]: v for k, v in npz.items() if k.startswith(prefix)}


def layout(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def load(module, npz, prefix):
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sub(npz, prefix + "sd.").items()}, strict=True)
    return module


def host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def check(npz, key, got, what=None):
    """the module rule of the docstring for the fixture entry `key`"""
    ref32, ref64 = npz[key].astype(np.float64), npz[key + "_f64"]
    got = host(got).astype(np.float64).reshape(ref64.shape)
    scale = max(float(np.abs(ref64).max()), 1e-30)
    e, dev = float(np.abs(ref32 - ref64).max()) / scale, float(np.abs(got - ref64).max()) / scale
    bound = FACTOR * e if e > 0 else FLOOR
    print("%s: reference float32 against float64 e = %.3e, device against float64 %.3e, bound %.3e" % (what or key, e, dev, bound))
    if not dev <= bound:
        MISSES.append((what or key, dev, bound))


def check_grads(npz, prefix, module):
    """The parameter gradients, tensor by tensor.  Some are zero in exact arithmetic: the bias of a BatchNorm whose output
    reaches another train-mode BatchNorm only through ReLUs that the fixture keeps in their linear range (a shift of it is a shift
    of the next BatchNorm's input, which that one removes), and a Conv bias in the same place.  The float64 run holds 1e-16 of
    the module's largest gradient there and both float32 runs hold rounding noise, so such a tensor has no magnitude of its own
    to be relative to; its values are exact, and the floor applies, against the largest gradient of the module."""
    grads = {k: p.grad for k, p in module.named_parameters()}
    largest = max(float(np.abs(npz[prefix + k + "_f64"]).max()) for k in grads)
    sizes = {k: float(np.abs(npz[prefix + k + "_f64"]).max()) / largest for k in grads}
    assert not any(1e-12 < v < 1e-7 for v in sizes.values()), sizes            # zero or not: nothing in between
    for k, g in grads.items():
        if sizes[k] <= 1e-12:
            ref32, dev = float(np.abs(npz[prefix + k]).max()) / largest, float(np.abs(host(g)).max()) / largest
            print("%s%s is zero in exact arithmetic: reference float32 %.3e, device %.3e of the largest gradient, floor %.0e"
                  % (prefix, k, ref32, dev, FLOOR))
            if not dev <= FLOOR:
                MISSES.append((prefix + k, dev, FLOOR))
        else:
            check(npz, prefix + k, g)


def settle():
    """every figure of a test is printed before the test asserts on them"""
    missed, MISSES[:] = list(MISSES), []
    assert not missed, missed


# ---- without a GPU --------------------------------------------------------------------------------------------------------
def test_state_dict_layout_is_the_references():
    from pdanet_amd.point_head import PointHeadBox
    from pdanet_amd.point_rcnn import PointRCNN
    from pdanet_amd.pointnet2_backbone import PointNet2MSG
    from pdanet_amd.pointrcnn_head import PointRCNNHead
    model_cfg, ds = CFG['MODEL'], CFG['dataset']
    before = json.dumps(CFG, sort_keys=True)
    backbone = PointNet2MSG(to_attr(model_cfg['BACKBONE_3D']), input_channels=4)
    assert layout(backbone) == FIXTURE['PointNet2MSG'] and backbone.num_point_features == 128
    point = PointHeadBox(num_class=3, input_channels=128, model_cfg=to_attr(model_cfg['POINT_HEAD']), predict_boxes_when_training=True)
    assert layout(point) == FIXTURE['PointHeadBox']
    head = PointRCNNHead(input_channels=128, model_cfg=to_attr(model_cfg['ROI_HEAD']), num_class=1)
    assert layout(head) == FIXTURE['PointRCNNHead']
    # USE_BN: False reaches xyz_up_layer and merge_down_layer only; the SA stack keeps its BatchNorm
    assert [type(m).__name__ for m in head.xyz_up_layer] == ['Conv2d', 'ReLU', 'Conv2d', 'ReLU']
    assert [type(m).__name__ for m in head.merge_down_layer] == ['Conv2d', 'ReLU'] and head.merge_down_layer[0].bias is not None
    assert [type(m).__name__ for m in head.SA_modules[0].mlps[0]][:3] == ['Conv2d', 'BatchNorm2d', 'ReLU']
    assert float(head.reg_layers[-1].weight.detach().std()) < 0.01 < float(head.cls_layers[-1].weight.detach().std())   # normal(0, 0.001)
    model = PointRCNN(to_attr(model_cfg), 3, ds)
    own = model.state_dict()
    assert [[k, list(v.shape)] for k, v in own.items()] == FIXTURE['PointRCNN']
    assert [n for n, _ in model.named_children()] == ['backbone_3d', 'point_head', 'roi_head']
    assert model.point_head.num_class == 3 and model.roi_head.num_class == 1 and model.point_head.predict_boxes_when_training
    sd = {k: torch.zeros(shape, dtype=own[k].dtype) for k, shape in FIXTURE['PointRCNN']}
    PointRCNN(to_attr(model_cfg), 3, ds).load_state_dict(sd, strict=True)
    assert json.dumps(CFG, sort_keys=True) == before                              # no module modified the config


def test_other_names_are_refused():
    from pdanet_amd.point_rcnn import PointRCNN
    for key, other in (('BACKBONE_3D', 'PointNet2Backbone'), ('POINT_HEAD', 'PointIntraPartOffsetHead'), ('POINT_HEAD', 'PointHeadSimple'),
                       ('ROI_HEAD', 'PartA2FCHead'), ('ROI_HEAD', 'PVRCNNHead')):
        cfg = json.loads(json.dumps(CFG['MODEL']))
        cfg[key]['NAME'] = other
        with pytest.raises(NotImplementedError, match=other):
            PointRCNN(to_attr(cfg), 3, CFG['dataset'])
    cfg = json.loads(json.dumps(CFG['MODEL']))
    del cfg['POINT_HEAD']
    with pytest.raises(ValueError, match="POINT_HEAD"):
        PointRCNN(to_attr(cfg), 3, CFG['dataset'])


def test_point_head_template_still_refuses_what_is_out_of_scope():
    from pdanet_amd.point_head import PointHeadBox
    head = PointHeadBox(num_class=3, input_channels=8, model_cfg=to_attr(CFG['MODEL']['POINT_HEAD']))
    pts, gt = torch.zeros(4, 4), torch.zeros(2, 1, 8)
    for kw in (dict(ret_part_labels=True), dict(use_ball_constraint=True), dict(set_ignore_flag=False)):
        with pytest.raises(NotImplementedError):
            head.assign_stack_targets(pts, gt, **kw)


def test_symbol_is_exported_and_bound():
    from pdanet_amd import build, _lib
    build.build()
    lib = _lib.load()
    assert hasattr(lib, SYMBOL) and SYMBOL in _lib.SIGNATURES
    assert lib.pda_abi_version() == 20


def test_argument_validation_without_gpu():
    from pdanet_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, SYMBOL)
    err = lambda: lib.pda_last_error()
    one = torch.zeros(8).data_ptr()
    call = lambda ptr=None, extra=None, b=2, n=10, m=3, c=4, s=16: fn(ptr, ptr, ptr, ptr, extra, 70.0, ptr, ptr, b, n, m, c, s, None)
    # sizes are checked before any pointer
    assert call(s=0) == 1 and b"bad size" in err()
    assert call(s=15361) == 1 and b"LDS" in err()
    assert call(c=-1) == 1 and b"bad size" in err()
    assert call(b=65536) == 1 and b"65535" in err()
    assert call() == 1 and b"null" in err()
    assert call(ptr=one) == 1 and b"null" in err()                      # the three host floats are a pointer too
    assert call(b=0) == 0 and call(m=0) == 0                             # an empty problem touches nothing


def test_wrapper_has_no_cpu_path():
    from pdanet_amd.roipoint_pool3d_utils import roipoint_pool3d_canonical
    with pytest.raises(RuntimeError, match="no CPU path"):
        roipoint_pool3d_canonical(torch.zeros(1, 4, 3), torch.zeros(1, 4), torch.zeros(1, 4, 2), torch.zeros(1, 2, 7), (0, 0, 0), 8, 70.0)
    with pytest.raises(ValueError):
        roipoint_pool3d_canonical(torch.zeros(1, 4, 3), torch.zeros(1, 4), torch.zeros(1, 4, 2), torch.zeros(2, 2, 7), (0, 0, 0), 8, 70.0)


@pytest.mark.parametrize("tag,kw", [("mean", {'use_mean_size': True, 'mean_size': [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]}),
                                    ("plain", {'use_mean_size': False})])
def test_point_residual_coder_matches_reference(npz, tag, kw):
    from pdanet_amd.box_coder_utils import PointResidualCoder
    coder = PointResidualCoder(**kw)
    assert coder.code_size == 8
    boxes, pts = torch.from_numpy(npz["coder_boxes"].copy()), torch.from_numpy(npz["coder_points"])
    classes = boxes[:, 7].long()
    codes = coder.encode_torch(boxes[:, :7], pts, classes)
    assert np.array_equal(boxes.numpy(), npz["coder_boxes"]) and (npz["coder_boxes"][0, 3:6] == 0).all()   # the clamp is on a copy
    check(npz, "coder_%s_codes" % tag, codes)
    check(npz, "coder_%s_decoded" % tag, coder.decode_torch(torch.from_numpy(npz["coder_%s_codes" % tag]), pts, classes))
    both = np.concatenate([boxes.numpy()[:, :7], np.ones((len(boxes), 2), np.float32)], axis=1)       # extra columns pass through
    assert np.array_equal(coder.encode_torch(torch.from_numpy(both), pts, classes).numpy()[:, 8:], both[:, 7:])
    settle()


# ---- the kernel against the composed path on the device -----------------------------------------------------------------------
S = 16


def inside(rng, roi, n):
    """n lattice points well inside a RoI"""
    u = (rng.random((n, 3)) - 0.5) * 0.8 * roi[3:6]
    c, s = np.cos(roi[6]), np.sin(roi[6])
    p = np.stack([u[:, 0] * c - u[:, 1] * s, u[:, 0] * s + u[:, 1] * c, u[:, 2]], axis=1) + roi[0:3]
    # + 0.0: no negative zero among the coordinates.  z' = dz keeps the sign of a zero, the composed path's matmul adds the
    # 0 * dx + 0 * dy of its third column to it and gives +0
    return np.round(p * 8) / 8 + 0.0


def pool_case(channels, flat=False):
    """B = 2, N = 300 (a walk crosses the 256-point tile), M = 6 RoIs a scene: more than S points, fewer than S on both sides of
    the tile boundary, empty, a zero padding row, a heading-0 box on the lattice, a rotated one.  flat: every heading is 0."""
    rng = np.random.default_rng(77 + channels)
    B, N, M = 2, 300, 6
    rois = np.zeros((B, M, 7), np.float32)
    xyz = np.zeros((B, N, 3), np.float32)
    for b in range(B):
        rois[b, 0] = [5.0, 0.5 * b, 0.0, 4.0, 2.0, 2.0, 0.3 + b]
        rois[b, 1] = [10.0, 5.0, 0.25, 1.0, 1.0, 1.0, 0.7 * b]
        rois[b, 2] = [-30.0, -30.0, 0.0, 2.0, 2.0, 2.0, 0.5]
        rois[b, 4] = [5.25, 0.5 * b, 0.0, 3.0, 1.5, 1.5, 0.0]
        rois[b, 5] = [5.0, 0.5 * b + 0.3, 0.1, 6.0, 1.0, 3.0, -2.5 + b]
        if flat:
            rois[b, :, 6] = 0
        pts = np.stack([rng.integers(160, 320, N), rng.integers(-80, 80, N), rng.integers(-16, 16, N)], axis=1) / 8.0
        big = rng.permutation(N)[:60]
        pts[big] = inside(rng, rois[b, 0], 60)
        small = np.array([3, 130, 255, 256, 299])
        pts[small] = inside(rng, rois[b, 1], 5)
        xyz[b] = pts
    idx = np.broadcast_to(np.arange(N, dtype=np.float32), (B, N))
    scores = np.ascontiguousarray(idx + 0.25)                                   # the point index, so the selection shows
    feats = rng.standard_normal((B, N, channels)).astype(np.float32)
    if channels:
        feats[:, :, 0] = idx
    return xyz, scores, feats, rois


def run_both(xyz, scores, feats, rois, extra=(0.0, 0.0, 0.0)):
    from pdanet_amd.roipoint_pool3d_utils import roipoint_pool3d_canonical, roipoint_pool3d_canonical_composed
    args = [torch.from_numpy(a).cuda() for a in (xyz, scores, feats, rois)]
    fused = roipoint_pool3d_canonical(*args, extra, S, 70.0)
    composed = roipoint_pool3d_canonical_composed(*args, extra, S, 70.0)
    assert not fused[0].requires_grad and fused[0].shape == composed[0].shape == (rois.shape[0], rois.shape[1], S, 5 + feats.shape[2])
    return [host(v) for v in fused], [host(v) for v in composed]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def compare_pools(got, ref, rois, exact_xyz):
    """got / ref: (pooled (B, M, S, 5 + C), flag (B, M)); exact_xyz (B, M) bool: where the canonical xyz must have the same bits"""
    (gp, gf), (rp_, rf) = got, ref
    assert np.array_equal(gf, rf)
    assert np.array_equal(bits(gp[..., 3]), bits(rp_[..., 3])) and np.array_equal(bits(gp[..., 5:]), bits(rp_[..., 5:]))
    d_xyz, d_depth = np.abs(gp[..., 0:3] - rp_[..., 0:3]), np.abs(gp[..., 4] - rp_[..., 4])
    print("canonical xyz: largest difference %.3e (bound %.0e), depth %.3e (bound %.0e)" % (d_xyz.max(), XYZ_TOL, d_depth.max(), DEPTH_TOL))
    assert d_xyz.max() <= XYZ_TOL and d_depth.max() <= DEPTH_TOL
    same = bits(gp[..., 0:3]) == bits(rp_[..., 0:3])
    for where in np.argwhere(~same & exact_xyz[:, :, None, None])[:8]:
        print("canonical xyz bits differ at", where.tolist(), repr(gp[tuple(where)]), repr(rp_[tuple(where)]))
    assert same[exact_xyz].all()
    assert (gp[gf > 0] == 0).all()


@gpu
@pytest.mark.parametrize("channels", [0, 8, 130])
def test_gpu_pool_against_the_composed_path(channels):
    xyz, scores, feats, rois = pool_case(channels)
    got, ref = run_both(xyz, scores, feats, rois)
    flag = got[1]
    assert flag[:, 2].all() and flag[:, 3].all() and not flag[:, [0, 1, 4, 5]].any()          # empty and zero padding rows
    compare_pools(got, ref, rois, exact_xyz=(rois[..., 6] == 0) & (flag == 0))
    # the selection itself: ascending point indices, slot k >= cnt repeating slot k % cnt
    picked = got[0][..., 3] - 0.25
    assert np.array_equal(picked[:, 1, :5], np.broadcast_to([3, 130, 255, 256, 299], (2, 5)))
    assert np.array_equal(picked[:, 1], picked[:, 1, np.arange(S) % 5])
    assert (np.diff(picked[:, 0], axis=1) > 0).all()                                         # more than S inside: the first S
    if channels:
        assert np.array_equal(got[0][..., 5][flag == 0], picked[flag == 0])
    again, _ = run_both(xyz, scores, feats, rois)
    assert np.array_equal(bits(again[0]), bits(got[0])) and np.array_equal(again[1], got[1])   # two runs give the same bits
    # enlarged RoIs: the float32 additions of enlarge_box3d
    got_w, ref_w = run_both(xyz, scores, feats, rois, extra=(0.5, 0.25, 1.0))
    compare_pools(got_w, ref_w, rois, exact_xyz=(rois[..., 6] == 0) & (got_w[1] == 0))


def raw_pool(xyz, scores, feats, rois, pooled, flag):
    from pdanet_amd.pointnet2_batch_cuda import _call
    b, n, m, c = xyz.shape[0], xyz.shape[1], rois.shape[1], feats.shape[2]
    extra = (ctypes.c_float * 3)(0, 0, 0)
    _call(SYMBOL, xyz, xyz.data_ptr(), scores.data_ptr(), feats.data_ptr(), rois.data_ptr(), extra, 70.0, pooled.data_ptr(),
          flag.data_ptr(), b, n, m, c, S)


@gpu
def test_gpu_pool_writes_all_of_its_output_and_survives_hostile_rows():
    xyz, scores, feats, rois = pool_case(8)
    clean, _ = run_both(xyz, scores, feats, rois)
    args = [torch.from_numpy(a).cuda() for a in (xyz, scores, feats, rois)]
    pooled = torch.full((2, 6, S, 13), float('nan'), device="cuda")
    flag = torch.full((2, 6), -7, dtype=torch.int32, device="cuda")
    raw_pool(*args, pooled, flag)
    assert np.array_equal(bits(host(pooled)), bits(clean[0])) and np.array_equal(host(flag), clean[1])   # NaN prefill: nothing is left
    hostile = rois.copy()
    hostile[0, 0] = np.nan
    hostile[0, 4] = np.inf
    hostile[1, 0, 6] = np.nan
    hostile[1, 5, 3] = -np.inf
    pooled.fill_(float('nan'))
    raw_pool(args[0], args[1], args[2], torch.from_numpy(hostile).cuda(), pooled, flag)
    got, gflag = host(pooled), host(flag)
    bad = ~np.isfinite(hostile).all(axis=-1)
    assert bad.sum() == 4 and gflag[bad].all() and (got[bad] == 0).all()
    assert np.array_equal(bits(got[~bad]), bits(clean[0][~bad])) and np.array_equal(gflag[~bad], clean[1][~bad])
    # no points at all: every RoI is empty
    from pdanet_amd.roipoint_pool3d_utils import roipoint_pool3d_canonical
    p0, f0 = roipoint_pool3d_canonical(args[0][:, :0], args[1][:, :0], args[2][:, :0], args[3], (0, 0, 0), S, 70.0)
    assert f0.all() and not p0.any()


def rh_pool_inputs(npz, rois):
    B = rois.shape[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return (t(npz["rh_coords"][:, 1:4].reshape(B, -1, 3)), t(npz["rh_scores"].reshape(B, -1)),
            t(npz["rh_features"].reshape(B, -1, npz["rh_features"].shape[-1])), t(rois))


@gpu
@pytest.mark.parametrize("which,rois_key", [("eval", "rh_rois"), ("train", "rh_t_rois")])
def test_gpu_pool_against_the_fixture(npz, which, rois_key):
    from pdanet_amd.roipoint_pool3d_utils import roipoint_pool3d_canonical
    rois = npz[rois_key]
    pooled, flag = roipoint_pool3d_canonical(*rh_pool_inputs(npz, rois), (0.0, 0.0, 0.0), S, 70.0)
    got, ref = host(pooled).reshape(-1, S, 13), npz["rh_pooled_" + which]
    assert np.array_equal(bits(got[..., 3]), bits(ref[..., 3])) and np.array_equal(bits(got[..., 5:]), bits(ref[..., 5:]))
    d_xyz, d_depth = np.abs(got[..., 0:3] - ref[..., 0:3]).max(), np.abs(got[..., 4] - ref[..., 4]).max()
    print("fixture %s: canonical xyz %.3e (bound %.0e), depth %.3e (bound %.0e)" % (which, d_xyz, XYZ_TOL, d_depth, DEPTH_TOL))
    assert d_xyz <= XYZ_TOL and d_depth <= DEPTH_TOL
    flat = (rois[..., 6] == 0).reshape(-1)
    assert flat.any() and np.array_equal(bits(got[flat][..., 0:3]), bits(ref[flat][..., 0:3]))
    empty = host(flag).reshape(-1) > 0
    assert np.array_equal(empty, ~ref.any(axis=(1, 2)))
    if which == "eval":
        assert empty.reshape(2, 6)[:, 4:].all() and not empty.reshape(2, 6)[:, :4].any()


# ---- the modules against the fixture ---------------------------------------------------------------------------------------
def cuda(npz, key):
    return torch.from_numpy(npz[key]).cuda()


@gpu
def test_gpu_sa_modules_against_the_reference(npz):
    from pdanet_amd.pointnet2_modules import PointnetSAModule, PointnetSAModuleMSG
    radii = npz["sa_radii"].tolist()
    msg = load(PointnetSAModuleMSG(npoint=32, radii=radii, nsamples=[8, 16], mlps=[[4, 8, 8], [4, 8, 16]], use_xyz=True), npz, "sa_msg_")
    one = load(PointnetSAModule(mlp=[4, 8, 16], npoint=None, radius=None, nsample=None, use_xyz=True), npz, "sa_all_")
    xyz, feat = cuda(npz, "sa_xyz"), cuda(npz, "sa_features")
    for tag, mod in (("msg", msg.cuda()), ("all", one.cuda())):
        mod.eval()
        with torch.no_grad():
            new_xyz, out = mod(xyz, feat)
        check(npz, "sa_%s_out_eval" % tag, out)
        mod.train()
        new_xyz, out = mod(xyz, feat)
        check(npz, "sa_%s_out_train" % tag, out)
        if tag == "msg":
            assert np.array_equal(bits(host(new_xyz)), bits(npz["sa_msg_new_xyz"]))          # the FPS picks
        else:
            assert new_xyz is None and out.shape == (2, 16, 1)
        for k, v in mod.named_buffers():
            if v.is_floating_point():
                check(npz, "sa_%s_after.%s" % (tag, k), v)
            else:
                assert int(v) == int(npz["sa_%s_after.%s" % (tag, k)])
    # the training form with a gradient: the narrow chains recompute, nothing grouped is kept
    msg.train()
    new_xyz, out = msg(xyz, feat.clone().requires_grad_(True))
    check(npz, "sa_msg_out_train", out, "sa msg train, features requiring grad")
    settle()


@gpu
def test_gpu_fp_module_against_the_reference(npz):
    from pdanet_amd.pointnet2_modules import PointnetFPModule
    mod = load(PointnetFPModule(mlp=[12, 16, 16]), npz, "fp_").cuda()
    args = [cuda(npz, k) for k in ("fp_unknown", "fp_known", "fp_unknow_feats", "fp_known_feats")]
    for mode in ("eval", "train"):
        mod.train(mode == "train")
        with torch.no_grad():
            check(npz, "fp_out_" + mode, mod(*args))
    settle()


@gpu
def test_gpu_backbone_against_the_reference(npz):
    from pdanet_amd.pointnet2_backbone import PointNet2MSG
    mod = load(PointNet2MSG(to_attr(json.loads(str(npz["bb_cfg"]))), input_channels=4), npz, "bb_").cuda()
    assert mod.num_point_features == 16
    for mode in ("eval", "train"):
        mod.train(mode == "train")
        with torch.no_grad():
            bd = mod({'batch_size': 2, 'points': cuda(npz, "bb_points")})
        check(npz, "bb_point_features_" + mode, bd['point_features'])
        assert np.array_equal(bits(host(bd['point_coords'])), bits(npz["bb_point_coords"]))
    mod.train()
    bd = mod({'batch_size': 2, 'points': cuda(npz, "bb_points")})                 # with gradients: the training forms
    check(npz, "bb_point_features_train", bd['point_features'], "bb point_features, training forms")
    bd['point_features'].sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in mod.parameters())
    settle()


def point_head(npz):
    from pdanet_amd.point_head import PointHeadBox
    cfg = json.loads(str(npz["ph_cfg"]))
    return load(PointHeadBox(num_class=3, input_channels=npz["ph_features"].shape[1], model_cfg=to_attr(cfg)), npz, "ph_").cuda()


def ph_batch(npz):
    return {'batch_size': 2, 'point_features': cuda(npz, "ph_features"), 'point_coords': cuda(npz, "ph_coords"),
            'gt_boxes': cuda(npz, "ph_gt_boxes")}


@gpu
def test_gpu_point_head_box_against_the_reference(npz):
    head = point_head(npz)
    head.eval()
    with torch.no_grad():
        bd = head(ph_batch(npz))
    assert bd['cls_preds_normalized'] is False and np.array_equal(host(bd['batch_index']), npz["ph_coords"][:, 0])
    check(npz, "ph_batch_cls_preds", bd['batch_cls_preds'])
    check(npz, "ph_batch_box_preds", bd['batch_box_preds'])
    check(npz, "ph_cls_scores_eval", bd['point_cls_scores'])
    head.train()
    gt = cuda(npz, "ph_gt_boxes")
    bd = head(dict(ph_batch(npz), gt_boxes=gt))
    assert 'batch_box_preds' not in bd                                            # no RoI head: nothing is decoded in training
    assert np.array_equal(host(gt), npz["ph_gt_boxes"])                          # the targets leave the boxes alone
    fr = head.forward_ret_dict
    labels = fr['point_cls_labels']
    assert labels.dtype == torch.int64 and np.array_equal(host(labels), npz["ph_labels"])
    assert int(labels[1]) == -1 and not host(labels)[96:].any()                  # the enlarged box only; a scene without foreground
    box_labels = host(fr['point_box_labels'])
    assert np.array_equal(box_labels != 0, npz["ph_box_labels"] != 0) and not box_labels[host(labels) <= 0].any()
    check(npz, "ph_box_labels", box_labels)
    check(npz, "ph_cls_preds", fr['point_cls_preds'])
    check(npz, "ph_box_preds", fr['point_box_preds'])
    loss, tb = head.get_loss()
    assert set(tb) == {'point_loss_cls', 'point_loss_box', 'point_pos_num'} and all(isinstance(v, torch.Tensor) and v.is_cuda for v in tb.values())
    check(npz, "ph_loss_cls", tb['point_loss_cls'])
    check(npz, "ph_loss_box", tb['point_loss_box'])
    loss.backward()
    check_grads(npz, "ph_grad.", head)
    head.predict_boxes_when_training = True
    bd = head(ph_batch(npz))
    assert bd['batch_box_preds'].shape == (192, 7) and bd['batch_cls_preds'].shape == (192, 3)
    settle()


def roi_head(npz):
    from pdanet_amd.pointrcnn_head import PointRCNNHead
    cfg = json.loads(str(npz["rh_cfg"]))
    return load(PointRCNNHead(input_channels=int(npz["rh_c_in"]), model_cfg=to_attr(cfg), num_class=1), npz, "rh_").cuda()


def rh_batch(npz, rois=None):
    rois = npz["rh_rois"] if rois is None else rois
    return {'batch_size': 2, 'rois': torch.from_numpy(rois).cuda(), 'roi_scores': cuda(npz, "rh_roi_scores"),
            'roi_labels': cuda(npz, "rh_roi_labels"), 'gt_boxes': cuda(npz, "rh_gt_boxes"), 'point_coords': cuda(npz, "rh_coords"),
            'point_features': cuda(npz, "rh_features"), 'point_cls_scores': cuda(npz, "rh_scores")}


def rh_draws(npz):
    return {k: npz["rh_" + k] for k in ('perm', 'fg_rand', 'hard_draw', 'easy_draw')}


@gpu
def test_gpu_roi_head_against_the_reference(npz, monkeypatch):
    from pdanet_amd import pointrcnn_head
    monkeypatch.setenv(pointrcnn_head.ENV, "fused")
    head = roi_head(npz)
    head.eval()
    with torch.no_grad():
        bd = head(rh_batch(npz))
    assert bd['cls_preds_normalized'] is False
    check(npz, "rh_batch_cls_preds", bd['batch_cls_preds'])
    check(npz, "rh_batch_box_preds", bd['batch_box_preds'])
    head.train()
    head(dict(rh_batch(npz), roi_target_draws=rh_draws(npz)))
    fr = head.forward_ret_dict
    assert np.array_equal(bits(host(fr['rois'])), bits(npz["rh_t_rois"]))        # the recorded draws sample the reference's RoIs
    assert np.array_equal(host(fr['rcnn_cls_labels']), npz["rh_t_rcnn_cls_labels"])
    check(npz, "rh_rcnn_cls", fr['rcnn_cls'])
    check(npz, "rh_rcnn_reg", fr['rcnn_reg'])
    loss, tb = head.get_loss()
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in tb.values())
    for k in ('rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner'):
        check(npz, "rh_" + k, tb[k])
    check(npz, "rh_loss", loss)
    loss.backward()
    check_grads(npz, "rh_grad.", head)
    settle()


@gpu
def test_gpu_roi_head_pooling_paths_agree(npz, monkeypatch):
    from pdanet_amd import pointrcnn_head
    head = roi_head(npz).eval()
    flat = npz["rh_rois"].copy()
    flat[..., 6] = 0                                                             # heading 0 on the lattice: the same canonical bits
    res = {}
    for path in ("fused", "composed"):
        monkeypatch.setenv(pointrcnn_head.ENV, path)
        with torch.no_grad():
            res[path] = (host(head(rh_batch(npz, flat))['batch_cls_preds']), host(head(rh_batch(npz, flat))['batch_box_preds']),
                         head(rh_batch(npz)))
    assert np.array_equal(bits(res["fused"][0]), bits(res["composed"][0])) and np.array_equal(bits(res["fused"][1]), bits(res["composed"][1]))
    for path in ("fused", "composed"):                                           # general headings: each path within the bound
        check(npz, "rh_batch_cls_preds", res[path][2]['batch_cls_preds'], "rh batch_cls_preds, %s pooling" % path)
        check(npz, "rh_batch_box_preds", res[path][2]['batch_box_preds'], "rh batch_box_preds, %s pooling" % path)
    settle()


@gpu
def test_gpu_train_steps_read_nothing_on_the_host(npz, monkeypatch):
    from pdanet_amd import pointrcnn_head
    monkeypatch.setenv(pointrcnn_head.ENV, "fused")
    head, point = roi_head(npz).train(), point_head(npz).train()
    point.predict_boxes_when_training = True
    rb, pb = rh_batch(npz), ph_batch(npz)

    def steps():
        head(dict(rb, roi_target_seed=11))
        loss, _ = head.get_loss()
        loss.backward()
        point(dict(pb))
        loss, _ = point.get_loss()
        loss.backward()

    steps()                                                                       # loads, caches and first-use paths
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode(2)
    try:
        steps()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for m in (head, point) for p in m.parameters())


def small_model_cfg(npz):
    roi = json.loads(str(npz["rh_cfg"]))
    roi['NMS_CONFIG']['TRAIN']['NMS_POST_MAXSIZE'] = 32
    roi['NMS_CONFIG']['TEST']['NMS_POST_MAXSIZE'] = 16
    return {'NAME': 'PointRCNN', 'BACKBONE_3D': json.loads(str(npz["bb_cfg"])), 'POINT_HEAD': json.loads(str(npz["ph_cfg"])),
            'ROI_HEAD': dict(roi, XYZ_UP_LAYER=[16, 16]),
            'POST_PROCESSING': CFG['MODEL']['POST_PROCESSING']}


@gpu
def test_gpu_pointrcnn_train_and_eval(npz):
    from pdanet_amd.point_rcnn import PointRCNN
    torch.manual_seed(4)
    model = PointRCNN(to_attr(small_model_cfg(npz)), 3, CFG['dataset']).cuda()
    assert model.roi_head.merge_down_layer[0].in_channels == 32                  # the backbone's 16 features beside the 16 of xyz_up_layer
    points = npz["bb_points"]                                                    # 2 x 256 points
    gt = np.zeros((2, 3, 8), np.float32)
    gt[0, 0] = list(points[5, 1:4]) + [3.9, 1.6, 1.56, 0.3, 1]
    gt[0, 1] = list(points[40, 1:4]) + [0.8, 0.6, 1.73, 1.2, 2]
    gt[1, 0] = list(points[256 + 9, 1:4]) + [1.76, 0.6, 1.73, -0.4, 3]
    batch = {'batch_size': 2, 'points': torch.from_numpy(points).cuda(), 'gt_boxes': torch.from_numpy(gt).cuda()}
    model.train()
    ret, tb, disp = model(dict(batch, roi_target_seed=5))
    assert torch.isfinite(ret['loss']) and disp == {}
    assert set(tb) == {'point_loss_cls', 'point_loss_box', 'point_pos_num', 'rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner', 'rcnn_loss'}
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in tb.values())
    assert float(ret['loss'].detach()) == pytest.approx(float(tb['point_loss_cls'] + tb['point_loss_box'] + tb['rcnn_loss']), rel=1e-5)
    assert model.roi_head.forward_ret_dict['rcnn_cls'].shape == (16, 1) and model.roi_head.forward_ret_dict['rcnn_reg'].shape == (16, 7)
    assert model.point_head.forward_ret_dict['point_cls_labels'].shape == (512,) and float(tb['point_pos_num']) > 0
    ret['loss'].backward()
    for name, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    model.eval()
    with torch.no_grad():
        pred_dicts, recall = model(dict(batch))
    assert len(pred_dicts) == 2 and set(pred_dicts[0]) == {'pred_boxes', 'pred_scores', 'pred_labels'}
    assert set(recall) == {'gt', 'roi_0.3', 'rcnn_0.3', 'roi_0.5', 'rcnn_0.5', 'roi_0.7', 'rcnn_0.7'}
