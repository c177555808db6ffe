"""StackSAModuleMSG, VoxelSetAbstraction, PointHeadSimple, PVRCNNHead and PVRCNN: the reference's state-dict layout, the closed
form of the fused scale's backward, and the device against the reference's own CPU run (tests/golden/pv_rcnn.npz, made by
make_pv_rcnn_golden.py) and float64 restatements.

Tolerance on the device, the rule and factor of test_second_net.py / test_voxel_rcnn.py: `dense_sa` below restates one
set-abstraction layer with plain torch indexing over the numpy ball query (golden/stack_sa_restatement.py), `dense_bev` the
bilinear interpolation; both run in float64 on the CPU.  The fixture holds the same compositions as the reference ran them in
float32 on the CPU; its error against float64 is measured here and the device may be off by 4 times that.  Figures are
max |a - ref| / max |ref| per tensor; all parameter gradients together, normalised by the largest reference gradient; the
running statistics together (TORCH_STATS_BOUND below says which of them the rule binds).  Every figure is printed."""
import copy
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from pdanet_amd.config import to_attr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import stack_sa_restatement as rs  # noqa: E402

gpu = pytest.mark.gpu
FACTOR = 4.0
PCR, VOXEL = [0.0, -4.0, -2.0, 8.0, 4.0, 2.0], [0.25, 0.25, 0.25]            # the fixture's geometry
with open(os.path.join(HERE, "golden", "pv_rcnn_state_dict.json")) as _f:
    FIXTURE = json.load(_f)
CFG = FIXTURE['config']


@pytest.fixture(scope="module")
def npz():
    with np.load(os.path.join(HERE, "golden", "pv_rcnn.npz")) as f:
        return {k: f[k] for k in f.files}


def sub(npz, prefix):
    return {k[len(prefix):]: v for k, v in npz.items() if k.startswith(prefix)}


def layout(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


# ---- without a GPU --------------------------------------------------------------------------------------------------------
def test_state_dict_layout_is_the_references():
    from pdanet_amd.point_head import PointHeadSimple
    from pdanet_amd.pv_rcnn import PVRCNN
    from pdanet_amd.pvrcnn_head import PVRCNNHead
    from pdanet_amd.voxel_set_abstraction import VoxelSetAbstraction
    y, ds = CFG['yaml'], CFG['dataset']
    before = json.dumps(CFG, sort_keys=True)
    vsa = VoxelSetAbstraction(to_attr(y['PFE']), ds['voxel_size'], ds['point_cloud_range'], num_bev_features=y['NUM_BEV_FEATURES'],
                              num_rawpoint_features=ds['num_point_features'])
    assert layout(vsa) == FIXTURE['VoxelSetAbstraction']
    assert (vsa.num_point_features, vsa.num_point_features_before_fusion) == (128, 640)
    point = PointHeadSimple(num_class=1, input_channels=vsa.num_point_features_before_fusion, model_cfg=to_attr(y['POINT_HEAD']))
    assert layout(point) == FIXTURE['PointHeadSimple']
    head = PVRCNNHead(input_channels=vsa.num_point_features, model_cfg=to_attr(y['ROI_HEAD']), num_class=1)
    assert layout(head) == FIXTURE['PVRCNNHead']
    model = PVRCNN(to_attr(CFG['MODEL']), 3, ds)
    own = model.state_dict()
    assert [[k, list(v.shape)] for k, v in own.items()] == FIXTURE['PVRCNN']
    assert [n for n, _ in model.named_children()] == ['vfe', 'backbone_3d', 'map_to_bev_module', 'pfe', 'backbone_2d', 'dense_head',
                                                      'point_head', 'roi_head']
    sd = {k: torch.zeros(shape, dtype=own[k].dtype) for k, shape in FIXTURE['PVRCNN']}
    PVRCNN(to_attr(CFG['MODEL']), 3, ds).load_state_dict(sd, strict=True)
    assert json.dumps(CFG, sort_keys=True) == before                              # no module modified the config


def test_what_is_not_built_raises():
    from pdanet_amd.pointnet2_stack_modules import VectorPoolAggregationModuleMSG, build_local_aggregation_module
    from pdanet_amd.pv_rcnn import PVRCNN
    from pdanet_amd.voxel_set_abstraction import VoxelSetAbstraction
    y, ds = CFG['yaml'], CFG['dataset']
    make = lambda cfg: VoxelSetAbstraction(to_attr(cfg), ds['voxel_size'], ds['point_cloud_range'], num_bev_features=256,
                                           num_rawpoint_features=4)
    cfg = json.loads(json.dumps(y['PFE']))
    cfg['SAMPLE_METHOD'] = 'SPC'
    with pytest.raises(NotImplementedError):
        make(cfg)
    cfg = json.loads(json.dumps(y['PFE']))
    cfg['SA_LAYER']['raw_points']['FILTER_NEIGHBOR_WITH_ROI'] = True
    with pytest.raises(NotImplementedError):
        make(cfg)
    with pytest.raises(NotImplementedError):
        VectorPoolAggregationModuleMSG(input_channels=16, config={})
    with pytest.raises(NotImplementedError):
        build_local_aggregation_module(16, to_attr({'NAME': 'VectorPoolAggregationModuleMSG', 'MSG_POST_MLPS': [32]}))
    cfg = json.loads(json.dumps(CFG['MODEL']))
    del cfg['POINT_HEAD']
    with pytest.raises(ValueError):
        PVRCNN(to_attr(cfg), 3, ds)


def test_stack_sa_symbols_exist():
    from pdanet_amd import build, _lib
    build.build()
    lib = _lib.load()
    for name in ("pda_stack_sa_scratch_doubles", "pda_stack_sa_moments", "pda_stack_sa_fwd", "pda_stack_sa_apply", "pda_stack_sa_bwd1",
                 "pda_stack_sa_bwd2", "pda_bev_interpolate_fwd", "pda_bev_interpolate_bwd"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.pda_stack_sa_scratch_doubles(55296, 64, 64, 16) > 0 and lib.pda_stack_sa_scratch_doubles(10, 64, 48, 16) == -1
    assert lib.pda_stack_sa_scratch_doubles(10, 64, 64, 256) == -1
    # sizes are checked before any pointer is used
    assert lib.pda_stack_sa_fwd(*([None] * 15), 2, 10, 10, 64, 24, 16, None) == 1 and b"bad size" in lib.pda_last_error()
    assert lib.pda_stack_sa_bwd2(*([None] * 13), (torch.zeros(1).double().data_ptr()), 2, 10, 10, 64, 16, None) == 1 \
        and b"null" in lib.pda_last_error()
    assert lib.pda_bev_interpolate_fwd(None, None, None, None, None, 0, 2, 8, 6, 5, None) == 0


def kernel_statement(f, rel, rows, empty, w1x, w2, gamma1, beta1, gamma2, beta2, stats, eps, grad_out):
    """What csrc/stack_sa.hip and pointnet2_stack_modules compute for one scale, in the dtype of the inputs with dense torch
    operations: the kernels' per-slot values and sums, the module's finish.  stats: None for batch statistics, else
    (mean1, var1, mean2, var2).  -> out, dict of gradients."""
    from pdanet_amd.pointnet2_stack_modules import batch_moments, bn_backward_constants, bn_scale_shift
    M, ns = rows.shape
    n = M * ns
    live = (~empty)[:, None, None]
    y1 = (f[rows] + rel @ w1x.t()) * live                                          # (M, ns, C1)
    mean1, var1 = batch_moments(torch.stack([y1.sum((0, 1)), (y1 * y1).sum((0, 1))]), n) if stats is None else stats[:2]
    s1, t1, istd1 = bn_scale_shift(gamma1, beta1, mean1, var1, eps)
    z1 = torch.relu(s1 * y1 + t1)
    y2 = z1 @ w2.t()                                                               # (M, ns, C2)
    mean2, var2 = batch_moments(torch.stack([y2.sum((0, 1)), (y2 * y2).sum((0, 1))]), n) if stats is None else stats[2:]
    s2, t2, istd2 = bn_scale_shift(gamma2, beta2, mean2, var2, eps)
    u = torch.where(gamma2 >= 0, y2.max(dim=1)[0], y2.min(dim=1)[0])               # (M, C2)
    a = (y2 == u[:, None, :]).float().argmax(dim=1)                                # the first slot that attains it
    out = torch.relu(s2 * u + t2)
    g = grad_out * (out > 0)
    dgamma2, dbeta2, a2, b2 = bn_backward_constants(g.sum(0), (g * u).sum(0), s2, mean2, istd2, n, stats is None)
    hit = torch.arange(ns)[None, :, None] == a[:, None, :]
    dy2 = hit * (s2 * g)[:, None, :] - a2 - b2 * y2
    dw2 = torch.einsum('msd,msc->dc', dy2, z1)
    e1 = (dy2 @ w2) * (z1 > 0)
    dgamma1, dbeta1, a1, b1 = bn_backward_constants(e1.sum((0, 1)), (e1 * y1).sum((0, 1)), s1, mean1, istd1, n, stats is None)
    dy1 = (s1 * e1 - a1 - b1 * y1) * live
    df = torch.zeros_like(f).index_add_(0, rows.reshape(-1), dy1.reshape(n, -1))
    dw1x = torch.einsum('msc,msk->ck', dy1, rel)
    return out, dict(dW1x=dw1x, dW2=dw2, dF=df, dgamma1=dgamma1, dbeta1=dbeta1, dgamma2=dgamma2, dbeta2=dbeta2)


@pytest.mark.parametrize("batch_stats", [True, False])
def test_closed_form_backward_equals_float64_autograd(batch_stats):
    """The two-pass closed form against autograd through two real BatchNorm2d layers and a max over the slots; slot lists with
    padded repeats, 20 % empty (all-zero) rows, BatchNorm weights of both signs."""
    g = torch.Generator().manual_seed(5)
    N, M, ns, C1, C2, eps = 150, 120, 16, 32, 16, 1e-5
    D = torch.float64
    f = torch.randn(N, C1, generator=g, dtype=D, requires_grad=True)
    rel = torch.randn(M, ns, 3, generator=g, dtype=D)
    rows = torch.randint(0, N, (M, ns), generator=g)
    rows[:, 6:] = rows[:, :1]                                                      # padded repeats of the first hit
    rel[:, 6:] = rel[:, :1]
    empty = torch.rand(M, generator=g) < 0.2
    rows[empty] = 0
    rel[empty] = 0
    w1x = torch.randn(C1, 3, generator=g, dtype=D, requires_grad=True)
    w2 = (torch.randn(C2, C1, generator=g, dtype=D) / C1 ** 0.5).requires_grad_(True)
    bn1, bn2 = torch.nn.BatchNorm2d(C1, eps=eps).double(), torch.nn.BatchNorm2d(C2, eps=eps).double()
    with torch.no_grad():
        for bn in (bn1, bn2):
            c = bn.num_features
            bn.weight.copy_((torch.rand(c, generator=g, dtype=D) + 0.5) * (torch.randint(0, 2, (c,), generator=g) * 2 - 1))
            bn.bias.copy_(torch.randn(c, generator=g, dtype=D) * 0.3)
            bn.running_mean.copy_(torch.randn(c, generator=g, dtype=D) * 0.1)
            bn.running_var.copy_(torch.rand(c, generator=g, dtype=D) + 0.5)
    grad_out = torch.randn(M, C2, generator=g, dtype=D)
    stats = None if batch_stats else (bn1.running_mean.clone(), bn1.running_var.clone(), bn2.running_mean.clone(), bn2.running_var.clone())
    bn1.train(batch_stats), bn2.train(batch_stats)
    y1 = (f[rows] + rel @ w1x.t()).masked_fill(empty[:, None, None], 0)
    x = torch.relu(bn1(y1.permute(2, 0, 1).unsqueeze(0)))                           # (1, C1, M, ns)
    x = torch.relu(bn2(torch.nn.functional.conv2d(x, w2[:, :, None, None])))
    ref_out = x.max(dim=-1)[0].squeeze(0).t()
    (ref_out * grad_out).sum().backward()
    ref = dict(dW1x=w1x.grad, dW2=w2.grad, dF=f.grad, dgamma1=bn1.weight.grad, dbeta1=bn1.bias.grad, dgamma2=bn2.weight.grad,
               dbeta2=bn2.bias.grad)
    with torch.no_grad():
        out, got = kernel_statement(f.detach(), rel, rows, empty, w1x.detach(), w2.detach(), bn1.weight.detach(), bn1.bias.detach(),
                                    bn2.weight.detach(), bn2.bias.detach(), stats, eps, grad_out)
    assert float((out - ref_out).abs().max()) <= 1e-12 * float(ref_out.abs().max())
    assert int((ref_out > 0).sum()) > 100 and bool((bn2.weight < 0).any()) and bool((bn2.weight > 0).any())
    for name in ref:
        err = float((got[name] - ref[name]).abs().max())
        print("closed form, batch_stats=%s, %s: max abs error %.2e of %.2e" % (batch_stats, name, err, float(ref[name].abs().max())))
        assert err <= 1e-11 * float(ref[name].abs().max()), name


# ---- the float64 restatements ---------------------------------------------------------------------------------------------
def dense_sa(layer, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None, **unused):
    """StackSAModuleMSG.forward on the CPU in the dtype of `layer`: the numpy ball query, torch indexing."""
    dtype = features.dtype
    cnt, new_cnt = xyz_batch_cnt.numpy(), new_xyz_batch_cnt.numpy()
    xyz32, new32 = xyz.float().contiguous(), new_xyz.float().contiguous()          # on the lattice: exact in either type
    start = torch.from_numpy(np.repeat(rs.starts(cnt), new_cnt))[:, None]
    outs = []
    for k, grouper in enumerate(layer.groupers):
        idx = np.zeros((new32.shape[0], grouper.nsample), np.int32)
        rs.ball_query(grouper.radius, grouper.nsample, new32.numpy(), new_cnt, xyz32.numpy(), cnt, idx)
        empty = torch.from_numpy(idx[:, 0] < 0)
        rows = torch.from_numpy(np.where(idx[:, :1] < 0, 0, idx)).long() + start
        rel = (xyz32[rows] - new32[:, None, :]).to(dtype)                          # the float32 difference
        x = torch.cat([rel, features[rows]], dim=-1).masked_fill(empty[:, None, None], 0)     # (M, ns, 3 + C)
        x = layer.mlps[k](x.permute(2, 0, 1).unsqueeze(0))                         # (1, C, M, ns)
        pooled = x.max(dim=-1)[0] if layer.pool_method == 'max_pool' else x.mean(dim=-1)
        outs.append(pooled.squeeze(0).t())
    return new_xyz, torch.cat(outs, dim=1)


def dense_bev(keypoints, bev, pcr, voxel, stride):
    """interpolate_from_bev_features in the dtype of `bev`; the map coordinates are the float32 expressions."""
    k32 = keypoints.float()
    x = ((k32[:, 1] - pcr[0]) / voxel[0] / stride)
    y = ((k32[:, 2] - pcr[1]) / voxel[1] / stride)
    H, W = bev.shape[2:]
    x0, y0 = torch.floor(x).long(), torch.floor(y).long()
    x1, y1 = (x0 + 1).clamp(0, W - 1), (y0 + 1).clamp(0, H - 1)
    x0, y0 = x0.clamp(0, W - 1), y0.clamp(0, H - 1)
    x, y = x.to(bev.dtype), y.to(bev.dtype)
    b = k32[:, 0].long()
    at = lambda yy, xx: bev[b, :, yy, xx]                                           # (M, C)
    wa, wb = (x1 - x) * (y1 - y), (x1 - x) * (y - y0)
    wc, wd = (x - x0) * (y1 - y), (x - x0) * (y - y0)
    return at(y0, x0) * wa[:, None] + at(y1, x0) * wb[:, None] + at(y0, x1) * wc[:, None] + at(y1, x1) * wd[:, None]


def rel(a, ref):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def together(got, ref):
    """one figure over a dict of tensors, normalised by the largest reference entry"""
    assert set(got) == set(ref)
    scale = max(float(np.abs(np.asarray(r, np.float64)).max()) for r in ref.values())
    return max(float(np.abs(np.asarray(got[k], np.float64) - np.asarray(ref[k], np.float64)).max()) for k in ref) / scale


def check(what, e_dev, e_gold):
    print("%s: device %.3e, reference in float32 on the CPU %.3e, ratio %.2f" % (what, e_dev, e_gold, e_dev / max(e_gold, 1e-300)))
    assert e_dev <= FACTOR * e_gold, what


def sa_module(npz, mlps=((16, 16, 16), (16, 64, 32)), pool_method='max_pool', load=True):
    from pdanet_amd.pointnet2_stack_modules import StackSAModuleMSG
    mod = StackSAModuleMSG(radii=npz["sa_radii"].tolist(), nsamples=[16, 32], mlps=[list(m) for m in mlps], use_xyz=True,
                           pool_method=pool_method)
    if load:
        mod.load_state_dict({k: torch.from_numpy(v) for k, v in sub(npz, "sa_sd.").items()}, strict=True)
    return mod


def sa_args(npz, device):
    t = lambda k: torch.from_numpy(npz[k]).to(device)
    return dict(xyz=t("sa_xyz"), xyz_batch_cnt=t("sa_xyz_cnt"), new_xyz=t("sa_new_xyz"), new_xyz_batch_cnt=t("sa_new_cnt"))


def train_step(mod, forward, features, grad_out):
    f = features.clone().requires_grad_(True)
    out = forward(features=f)[1]
    (out * grad_out).sum().backward()
    grads = {k: p.grad.detach().cpu().numpy() for k, p in mod.named_parameters()}
    stats = {k: v.detach().cpu().numpy() for k, v in mod.named_buffers() if 'running' in k}
    return out.detach(), f.grad.detach(), grads, stats


# The statistics torch's own BatchNorm launches leave on the device (the composed path) are not this project's arithmetic and
# the 4x rule does not bind them: the CPU accumulates them in float64.  A float32 sum of n terms in any order is within
# (n - 1) 2^-24 of the exact sum relative to the sum of magnitudes; a batch mean and a batch variance are two such sums and the
# momentum update adds three roundings.  n = 303 x 32 slots is the most a layer of the fixture sees.
TORCH_STATS_BOUND = (2 * 303 * 32 + 3) * 2.0 ** -24


@pytest.fixture(scope="module")
def sa_truth(npz):
    """The float64 restatement of the set-abstraction module, once: eval output, train output, gradients, running statistics."""
    mod = sa_module(npz).double()
    args = sa_args(npz, "cpu")
    feat, grad_out = torch.from_numpy(npz["sa_features"]).double(), torch.from_numpy(npz["sa_grad_out"]).double()
    mod.eval()
    with torch.no_grad():
        out_eval = dense_sa(mod, features=feat, **args)[1]
    mod.train()
    out, gf, grads, stats = train_step(mod, functools.partial(dense_sa, mod, **args), feat, grad_out)
    gold_stats = {k: v for k, v in sub(npz, "sa_after.").items() if 'running' in k}
    return dict(out_eval=out_eval, out=out, grad_features=gf, grads=grads, stats=stats,
                e_gold=dict(out_eval=rel(npz["sa_out_eval"], out_eval), out=rel(npz["sa_out_train"], out),
                            grad_features=rel(npz["sa_grad_features"], gf), grads=together(sub(npz, "sa_grad."), grads),
                            stats=together(gold_stats, stats)))


def vsa_module(npz):
    from pdanet_amd.voxel_set_abstraction import VoxelSetAbstraction
    mod = VoxelSetAbstraction(to_attr(json.loads(str(npz["vsa_cfg"]))), VOXEL, PCR, num_bev_features=npz["vsa_bev"].shape[1],
                              num_rawpoint_features=4)
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in sub(npz, "vsa_sd.").items()}, strict=True)
    return mod


def vsa_batch(npz, device, dtype):
    from pdanet_amd.spconv_utils import SparseConvTensor
    feats = {name: SparseConvTensor(torch.from_numpy(npz["vsa_%s_features" % name]).to(device=device, dtype=dtype),
                                    torch.from_numpy(npz["vsa_%s_indices" % name]).to(device),
                                    npz["vsa_%s_spatial_shape" % name].tolist(), 2) for name in ("x_conv1", "x_conv2")}
    return {'batch_size': 2, 'points': torch.from_numpy(npz["vsa_points"]).to(device=device, dtype=dtype),
            'multi_scale_3d_features': feats, 'spatial_features': torch.from_numpy(npz["vsa_bev"]).to(device=device, dtype=dtype),
            'spatial_features_stride': 4}


def vsa_outputs(mod, batch_of):
    res = {}
    for mode in ("eval", "train"):                       # eval first: the train pass moves the running statistics
        mod.train(mode == "train")
        with torch.no_grad():
            bd = mod(batch_of())
        res["before_fusion_" + mode], res["point_features_" + mode] = bd['point_features_before_fusion'], bd['point_features']
    res["point_coords"] = bd['point_coords']
    return res


@pytest.fixture(scope="module")
def vsa_truth(npz):
    """VoxelSetAbstraction in float64 on the CPU: its layers replaced by dense_sa, the interpolation by dense_bev, the keypoints
    taken from the numpy farthest-point sampling."""
    mod = vsa_module(npz).double()
    for layer in list(mod.SA_layers) + [mod.SA_rawpoints]:
        layer.forward = functools.partial(dense_sa, layer)
    mod.interpolate_from_bev_features = lambda kp, bev, batch_size, bev_stride: dense_bev(kp, bev, PCR, VOXEL, bev_stride)
    points = npz["vsa_points"]
    counts = np.bincount(points[:, 0].astype(np.int64))
    rows = []
    for b, n in enumerate(counts):
        first = rs.fps(points[points[:, 0] == b][:, 1:4], min(int(n), 64), block=1024)    # the stacked kernel's tie rule
        rows.append(int(counts[:b].sum()) + first[np.arange(64) % len(first)])
    rows = np.stack(rows).astype(np.int64)
    keypoints = torch.from_numpy(np.concatenate([np.repeat(np.arange(2.0), 64)[:, None], points[rows.reshape(-1), 1:4]], axis=1))
    mod.get_sampled_points = lambda batch_dict: keypoints.double()
    res = vsa_outputs(mod, functools.partial(vsa_batch, npz, "cpu", torch.float64))
    res["rows"] = rows
    return res


HEAD_KEYS = ('pooled_eval', 'batch_cls_preds', 'batch_box_preds', 'pooled_train', 'rcnn_cls_train', 'rcnn_reg_train')


def head_module(npz):
    from pdanet_amd.pvrcnn_head import PVRCNNHead
    head = PVRCNNHead(input_channels=int(npz["head_c_in"]), model_cfg=to_attr(json.loads(str(npz["head_cfg"]))), num_class=1)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sub(npz, "head_sd.").items()}, strict=True)
    return head


def head_batch(npz, device, dtype):
    t = lambda k: torch.from_numpy(npz[k]).to(device=device, dtype=dtype)
    rois = t("head_rois")                                 # on the 1/8 lattice: exact in either type
    return {'batch_size': 2, 'rois': rois, 'roi_scores': torch.zeros(rois.shape[:2], device=device),
            'roi_labels': torch.ones(rois.shape[:2], dtype=torch.long, device=device), 'point_coords': t("head_point_coords"),
            'point_features': t("head_point_features"), 'point_cls_scores': t("head_point_cls_scores")}


def head_outputs(head, npz, device, dtype):
    """eval: pooled, batch_cls_preds, batch_box_preds through forward(); train: pooled and the two predictions."""
    res = {}
    head.eval()
    with torch.no_grad():
        res['pooled_eval'] = head.roi_grid_pool(head_batch(npz, device, dtype))
        bd = head(head_batch(npz, device, dtype))
        res['batch_cls_preds'], res['batch_box_preds'] = bd['batch_cls_preds'], bd['batch_box_preds']
    head.train()
    with torch.no_grad():
        pooled = head.roi_grid_pool(head_batch(npz, device, dtype))
        shared = head.shared_fc_layer(pooled.permute(0, 2, 1).contiguous().view(pooled.shape[0], -1, 1))
        res['pooled_train'] = pooled
        res['rcnn_cls_train'] = head.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        res['rcnn_reg_train'] = head.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
    return res


@pytest.fixture(scope="module")
def head_truth(npz):
    head = head_module(npz).double()
    head.roi_grid_pool_layer.forward = functools.partial(dense_sa, head.roi_grid_pool_layer)
    return head_outputs(head, npz, "cpu", torch.float64)


def bev_run(npz, device, dtype, interpolate):
    bev = torch.from_numpy(npz["bev_map"]).to(device=device, dtype=dtype).requires_grad_(True)
    kp = torch.from_numpy(npz["bev_keypoints"]).to(device=device, dtype=dtype)
    out = interpolate(kp, bev)
    (out * torch.from_numpy(npz["bev_grad_out"]).to(device=device, dtype=dtype)).sum().backward()
    return out.detach(), bev.grad.detach()


@pytest.fixture(scope="module")
def bev_truth(npz):
    return bev_run(npz, "cpu", torch.float64,
                   lambda kp, bev: dense_bev(kp, bev, npz["bev_pcr"].tolist(), npz["bev_voxel"].tolist(), int(npz["bev_stride"])))


def test_restatements_agree_with_the_reference_run(npz, sa_truth, bev_truth, vsa_truth, head_truth):
    """The fixture is the reference's own float32 run; the float64 restatements must be the same functions."""
    figures = {"sa " + k: e for k, e in sa_truth['e_gold'].items()}
    figures["bev values"], figures["bev map gradient"] = rel(npz["bev_out"], bev_truth[0]), rel(npz["bev_grad_map"], bev_truth[1])
    figures.update({"head " + k: rel(npz["head_" + k], head_truth[k]) for k in HEAD_KEYS})
    figures.update({"vsa " + k: rel(npz["vsa_" + k], vsa_truth[k]) for k in vsa_truth if k != "rows"})
    for k, e in figures.items():
        print("reference in float32 against the float64 restatement, %s: %.3e" % (k, e))
        assert e < 2e-4, k
    assert np.array_equal(vsa_truth["rows"], npz["vsa_keypoint_rows"])
    for k in ("mlps.0.4.weight", "mlps.1.4.weight"):                               # both signs: ymax and ymin are exercised
        assert (npz["sa_sd." + k] > 0).any() and (npz["sa_sd." + k] < 0).any()
    kp = npz["bev_keypoints"]
    x, y = kp[:, 1] * 2, (kp[:, 2] + 1.5) * 2                                      # the fixture's map coordinates
    assert (x < 0).any() and (x > 4).any() and (y < 0).any() and (y > 5).any() and ((x == np.floor(x)) & (y == np.floor(y))).any()


# ---- on the GPU -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("path", ["fused", "composed"])
def test_gpu_sa_module_against_the_reference(npz, sa_truth, path, monkeypatch):
    from pdanet_amd import pointnet2_stack_modules as psm
    monkeypatch.setenv(psm.ENV, path)
    mod = sa_module(npz).cuda()
    assert mod.is_fused(0) == mod.is_fused(1) == (path == "fused")
    args = sa_args(npz, "cuda")
    feat, grad_out = torch.from_numpy(npz["sa_features"]).cuda(), torch.from_numpy(npz["sa_grad_out"]).cuda()
    gold = sa_truth['e_gold']
    mod.eval()
    with torch.no_grad():
        check(path + " eval output", rel(mod(features=feat, **args)[1], sa_truth['out_eval']), gold['out_eval'])
    mod.train()
    out, gf, grads, stats = train_step(mod, functools.partial(mod, **args), feat, grad_out)
    check(path + " train output", rel(out, sa_truth['out']), gold['out'])
    check(path + " feature gradient", rel(gf, sa_truth['grad_features']), gold['grad_features'])
    check(path + " parameter gradients", together(grads, sa_truth['grads']), gold['grads'])
    e_stats = together(stats, sa_truth['stats'])
    if path == "fused":
        check("fused running statistics", e_stats, gold['stats'])
    else:
        print("composed running statistics: device %.3e, float32 summation bound %.3e" % (e_stats, TORCH_STATS_BOUND))
        assert e_stats <= TORCH_STATS_BOUND
    assert all(int(v) == 1 for k, v in mod.named_buffers() if k.endswith('num_batches_tracked'))
    if path == "fused":                                    # no centres: zeros of the right shape, nothing launched on the slots
        none = dict(args, new_xyz=args['new_xyz'][:0], new_xyz_batch_cnt=torch.zeros_like(args['new_xyz_batch_cnt']))
        f = feat.clone().requires_grad_(True)
        empty_out = mod(features=f, **none)[1]
        empty_out.sum().backward()
        assert empty_out.shape == (0, 48) and not f.grad.any()


@gpu
def test_gpu_fused_equals_composed_and_repeats_itself(npz, sa_truth, monkeypatch):
    from pdanet_amd import pointnet2_stack_modules as psm
    args = sa_args(npz, "cuda")
    feat, grad_out = torch.from_numpy(npz["sa_features"]).cuda(), torch.from_numpy(npz["sa_grad_out"]).cuda()
    res = {}
    for path in ("fused", "composed", "fused again"):
        monkeypatch.setenv(psm.ENV, path.split()[0])
        mod = sa_module(npz).cuda().train()
        res[path] = train_step(mod, functools.partial(mod, **args), feat, grad_out)
    gold = sa_truth['e_gold']
    (out_f, gf_f, grads_f, stats_f), (out_c, gf_c, grads_c, stats_c) = res["fused"], res["composed"]
    check("fused against composed, output", rel(out_f, out_c), gold['out'])
    check("fused against composed, feature gradient", rel(gf_f, gf_c), gold['grad_features'])
    check("fused against composed, parameter gradients", together(grads_f, grads_c), gold['grads'])
    e_stats = together(stats_f, stats_c)
    print("fused against composed, running statistics: %.3e, float32 summation bound %.3e" % (e_stats, TORCH_STATS_BOUND))
    assert e_stats <= TORCH_STATS_BOUND
    # Everything but dF (float atomics) is the same bits from run to run.  The feature columns of the first conv's weight
    # gradient are autograd's dF^T features, downstream of dF: they are compared under the rule, every other entry bit by bit.
    out_2, gf_2, grads_2, stats_2 = res["fused again"]
    assert torch.equal(out_f, out_2)
    for k in grads_f:
        first_conv = k.endswith('.0.weight')
        a, b = (grads_f[k][:, :3], grads_2[k][:, :3]) if first_conv else (grads_f[k], grads_2[k])
        assert np.array_equal(a, b), k
    for k in stats_f:
        assert np.array_equal(stats_f[k], stats_2[k]), k
    check("fused twice, parameter gradients downstream of dF", together(grads_f, grads_2), gold['grads'])
    check("fused twice, feature gradient", rel(gf_f, gf_2), gold['grad_features'])
    monkeypatch.setenv(psm.ENV, "neither")
    with pytest.raises(ValueError):
        mod(features=feat, **args)


@gpu
@pytest.mark.parametrize("case", ["three layers", "avg_pool"])
def test_gpu_composed_serves_what_the_fused_kernels_do_not(npz, case, monkeypatch):
    from pdanet_amd import pointnet2_stack_modules as psm
    monkeypatch.setenv(psm.ENV, "fused")
    torch.manual_seed(2)
    if case == "three layers":
        mod = sa_module(npz, mlps=((16, 16, 16, 16), (16, 32, 32)), load=False)
        assert not mod.is_fused(0) and mod.is_fused(1)
    else:
        mod = sa_module(npz, pool_method='avg_pool', load=False)
        assert not mod.is_fused(0) and not mod.is_fused(1)
    truth = copy.deepcopy(mod).double()
    mod = mod.cuda()
    feat, grad_out = torch.from_numpy(npz["sa_features"]), torch.from_numpy(npz["sa_grad_out"])
    out, gf, grads, _ = train_step(mod, functools.partial(mod, **sa_args(npz, "cuda")), feat.cuda(), grad_out.cuda())
    t_out, t_gf, t_grads, _ = train_step(truth, functools.partial(dense_sa, truth, **sa_args(npz, "cpu")), feat.double(), grad_out.double())
    # random parameters: ReLU masks near zero may differ, so this is a statement that the path runs and computes the layer, at
    # float32 accuracy for the output (continuous in the masks) and loosely for the gradients
    print("%s: output %.3e, feature gradient %.3e, parameter gradients %.3e" % (case, rel(out, t_out), rel(gf, t_gf), together(grads, t_grads)))
    assert out.shape == (303, 48) and rel(out, t_out) < 1e-5 and rel(gf, t_gf) < 1e-2 and together(grads, t_grads) < 1e-2


@gpu
def test_gpu_bev_interpolation_against_the_reference(npz, bev_truth):
    from pdanet_amd.voxel_set_abstraction import VoxelSetAbstraction
    obj = VoxelSetAbstraction.__new__(VoxelSetAbstraction)
    obj.point_cloud_range, obj.voxel_size = npz["bev_pcr"].tolist(), npz["bev_voxel"].tolist()
    out, grad = bev_run(npz, "cuda", torch.float32,
                        lambda kp, bev: VoxelSetAbstraction.interpolate_from_bev_features(obj, kp, bev, 2, int(npz["bev_stride"])))
    check("bev values", rel(out, bev_truth[0]), rel(npz["bev_out"], bev_truth[0]))
    check("bev map gradient", rel(grad, bev_truth[1]), rel(npz["bev_grad_map"], bev_truth[1]))
    kp = torch.from_numpy(npz["bev_keypoints"]).cuda()
    kp[::2, 0] = 7                                         # a batch index outside [0, B) reads and writes nothing
    bev = torch.from_numpy(npz["bev_map"]).cuda().requires_grad_(True)
    res = VoxelSetAbstraction.interpolate_from_bev_features(obj, kp, bev, 2, int(npz["bev_stride"]))
    res.sum().backward()
    assert not res[::2].any() and torch.equal(res[1::2], out[1::2]) and torch.isfinite(bev.grad).all()


@gpu
def test_gpu_voxel_set_abstraction_against_the_reference(npz, vsa_truth):
    mod = vsa_module(npz).cuda()
    mod.eval()
    keypoints, rows = mod.get_sampled_points(vsa_batch(npz, "cuda", torch.float32), return_indices=True)
    assert np.array_equal(rows.cpu().numpy(), npz["vsa_keypoint_rows"])              # scene 1 repeats its 32 samples
    assert np.array_equal(keypoints.cpu().numpy(), npz["vsa_point_coords"])
    got = vsa_outputs(mod, functools.partial(vsa_batch, npz, "cuda", torch.float32))
    for k in ("before_fusion_eval", "point_features_eval", "before_fusion_train", "point_features_train"):
        check("vsa " + k, rel(got[k], vsa_truth[k]), rel(npz["vsa_" + k], vsa_truth[k]))


@gpu
def test_gpu_point_head_against_the_reference(npz):
    from pdanet_amd.point_head import PointHeadSimple
    cfg = json.loads(str(npz["point_cfg"]))

    def make():
        head = PointHeadSimple(num_class=1, input_channels=npz["point_features"].shape[1], model_cfg=to_attr(cfg))
        head.load_state_dict({k: torch.from_numpy(v) for k, v in sub(npz, "point_sd.").items()}, strict=True)
        return head.train()

    truth = make().double()
    preds = truth.cls_layers(torch.from_numpy(npz["point_features"]).double())
    truth.forward_ret_dict = {'point_cls_preds': preds, 'point_cls_labels': torch.from_numpy(npz["point_labels"])}
    t_loss, _ = truth.get_loss()
    head = make().cuda()
    t = lambda k: torch.from_numpy(npz[k]).cuda()
    bd = head({'batch_size': 2, 'point_features_before_fusion': t("point_features"), 'point_coords': t("point_coords"),
               'gt_boxes': t("point_gt_boxes")})
    labels = head.forward_ret_dict['point_cls_labels']
    assert labels.dtype == torch.int64 and np.array_equal(labels.cpu().numpy(), npz["point_labels"])
    assert int(labels[1]) == -1                            # the point that lies in the enlarged box only
    loss, tb = head.get_loss()
    assert isinstance(tb['point_loss_cls'], torch.Tensor) and tb['point_loss_cls'].is_cuda and float(tb['point_pos_num']) == float((npz["point_labels"] > 0).sum())
    check("point head logits", rel(head.forward_ret_dict['point_cls_preds'], preds), rel(npz["point_cls_preds"], preds))
    check("point head scores", rel(bd['point_cls_scores'], torch.sigmoid(preds).max(dim=-1)[0]),
          rel(npz["point_cls_scores"], torch.sigmoid(preds).max(dim=-1)[0]))
    check("point head loss", rel(loss.reshape(1), t_loss.reshape(1)), rel(npz["point_loss"].reshape(1), t_loss.reshape(1)))


@gpu
def test_gpu_head_against_the_reference(npz, head_truth):
    got = head_outputs(head_module(npz).cuda(), npz, "cuda", torch.float32)
    assert got['pooled_train'].shape == (10, 27, 32) and got['batch_box_preds'].shape == (2, 5, 7)
    for k in HEAD_KEYS:
        check("head " + k, rel(got[k], head_truth[k]), rel(npz["head_" + k], head_truth[k]))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@gpu
def test_gpu_pv_rcnn_train_and_eval():
    from pdanet_amd.pv_rcnn import PVRCNN
    from pdanet_amd.voxel_utils import VoxelGenerator, collate_voxels
    ds = CFG['dataset']
    B = 2
    torch.manual_seed(3)
    model = PVRCNN(to_attr(CFG['MODEL']), 3, ds).cuda()
    rng = np.random.default_rng(5)
    pcr = np.array(ds['point_cloud_range'], np.float64)
    counts = [1500, 900]
    pts = np.concatenate([np.concatenate([rng.uniform(pcr[:3], pcr[3:], (n, 3)), rng.random((n, 1))], axis=1) for n in counts])
    offs = torch.tensor([0, counts[0], sum(counts)], dtype=torch.int64).cuda()
    gen = VoxelGenerator(ds['voxel_size'], ds['point_cloud_range'], 4, 5, 2000)
    voxels_, coords, num_points = collate_voxels(*gen.generate_batch((dev(pts.astype(np.float32)), offs, max(counts))))
    points = np.concatenate([np.repeat(np.arange(B), counts)[:, None], pts], axis=1).astype(np.float32)
    gt = np.zeros((B, 3, 8), np.float32)
    gt[0, 0] = [0.4, 0.0, -1.0, 3.9, 1.6, 1.56, 0.3, 1]
    gt[0, 1] = [0.3, 0.1, -0.6, 0.8, 0.6, 1.73, 1.2, 2]
    gt[1, 0] = [0.5, -0.1, -0.6, 1.76, 0.6, 1.73, -0.4, 3]
    roi_cfg = CFG['MODEL']['ROI_HEAD']
    n_rois, per_image = roi_cfg['NMS_CONFIG']['TRAIN']['NMS_POST_MAXSIZE'], roi_cfg['TARGET_CONFIG']['ROI_PER_IMAGE']
    # explicit draws, valid whatever the counts (test_voxel_rcnn.py): the identity permutation of the foreground list,
    # easy-background picks among the zero-padded RoI rows, hard-background pick 0
    draws = {'perm': [np.arange(n_rois)] * B, 'fg_rand': rng.random((B, per_image)), 'hard_draw': np.zeros((B, per_image), np.int64),
             'easy_draw': rng.integers(0, n_rois - 16, (B, per_image))}
    batch = {'voxels': voxels_, 'voxel_coords': coords, 'voxel_num_points': num_points, 'points': dev(points), 'gt_boxes': dev(gt),
             'batch_size': B}
    model.train()
    ret, tb, disp = model(dict(batch, roi_target_draws=draws))
    assert torch.isfinite(ret['loss']) and disp == {}
    assert set(tb) == {'loss_rpn', 'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir', 'rpn_loss', 'point_loss_cls', 'point_pos_num',
                       'rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner', 'rcnn_loss'}
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in tb.values())
    assert float(ret['loss'].detach()) == pytest.approx(float(tb['loss_rpn'] + tb['point_loss_cls'] + tb['rcnn_loss']), rel=1e-5)
    assert model.roi_head.forward_ret_dict['rcnn_cls'].shape == (B * per_image, 1)
    assert model.point_head.forward_ret_dict['point_cls_labels'].shape == (B * 2048,)
    ret['loss'].backward()
    for name, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    model.eval()
    with torch.no_grad():
        pred_dicts, recall = model(dict(batch))
        assert len(pred_dicts) == B and set(pred_dicts[0]) == {'pred_boxes', 'pred_scores', 'pred_labels'}
        assert set(recall) == {'gt', 'roi_0.3', 'rcnn_0.3', 'roi_0.5', 'rcnn_0.5', 'roi_0.7', 'rcnn_0.7'}
