"""NeighborVoxelSAModuleMSG, VoxelRCNNHead and VoxelRCNN: the reference's state-dict layout, the moment form of the position
BatchNorm, and the device against the reference's own CPU run (tests/golden/voxel_rcnn.npz, made by
make_voxel_rcnn_golden.py) and a float64 restatement.

Tolerance on the device, the rule and factor of test_second_net.py: `dense_pool` below restates one pooling layer with plain
torch indexing over the numpy voxel query (golden/stack_pool_restatement.py) and runs in float64 on the CPU.  The fixture holds
the same composition as the reference ran it in float32 on the CPU; its error against float64 is measured here and the device
may be off by 4 times that.  Figures are max |a - ref| / max |ref| per tensor; all parameter gradients together, normalised
by the largest reference gradient; the running statistics together (TORCH_STATS_BOUND below says which of them the rule
binds).  Every figure is printed."""
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
import stack_pool_restatement as rs  # noqa: E402

gpu = pytest.mark.gpu
FACTOR = 4.0
BACKBONE_CHANNELS = {'x_conv1': 16, 'x_conv2': 32, 'x_conv3': 64, 'x_conv4': 64}
PCR, VOXEL = [0.0, -4.0, -2.0, 8.0, 4.0, 2.0], [0.25, 0.25, 0.25]            # the fixture's geometry
with open(os.path.join(HERE, "golden", "voxel_rcnn_state_dict.json")) as _f:
    FIXTURE = json.load(_f)
CFG = FIXTURE['config']


@pytest.fixture(scope="module")
def npz():
    with np.load(os.path.join(HERE, "golden", "voxel_rcnn.npz")) as f:
        return {k: f[k] for k in f.files}


# ---- without a GPU --------------------------------------------------------------------------------------------------------
def test_state_dict_layout_is_the_references():
    from pdanet_amd.voxel_rcnn import VoxelRCNN
    from pdanet_amd.voxelrcnn_head import VoxelRCNNHead
    roi_cfg = CFG['MODEL']['ROI_HEAD']
    before = json.dumps(roi_cfg, sort_keys=True)
    head = VoxelRCNNHead(BACKBONE_CHANNELS, to_attr(roi_cfg), CFG['dataset']['point_cloud_range'], CFG['dataset']['voxel_size'], 1)
    assert [[k, list(v.shape)] for k, v in head.state_dict().items()] == FIXTURE['VoxelRCNNHead']
    assert json.dumps(roi_cfg, sort_keys=True) == before                          # the config is not modified
    model = VoxelRCNN(to_attr(CFG['MODEL']), 3, CFG['dataset'])
    own = model.state_dict()
    assert [[k, list(v.shape)] for k, v in own.items()] == FIXTURE['VoxelRCNN']
    assert [n for n, _ in model.named_children()] == ['vfe', 'backbone_3d', 'map_to_bev_module', 'backbone_2d', 'dense_head', 'roi_head']
    sd = {k: torch.zeros(shape, dtype=own[k].dtype) for k, shape in FIXTURE['VoxelRCNN']}
    VoxelRCNN(to_attr(CFG['MODEL']), 3, CFG['dataset']).load_state_dict(sd, strict=True)


def test_detectors_without_a_roi_head_table_refuse_the_block():
    from pdanet_amd.second_net import SECONDNet
    from pdanet_amd.voxel_rcnn import VoxelRCNN
    with pytest.raises(NotImplementedError):
        SECONDNet(to_attr(CFG['MODEL']), 3, CFG['dataset'])
    cfg = json.loads(json.dumps(CFG['MODEL']))
    cfg['ROI_HEAD']['NAME'] = 'PVRCNNHead'
    with pytest.raises(NotImplementedError):
        VoxelRCNN(to_attr(cfg), 3, CFG['dataset'])
    del cfg['ROI_HEAD']
    with pytest.raises(ValueError):
        VoxelRCNN(to_attr(cfg), 3, CFG['dataset'])


def test_voxel_pool_symbols_exist():
    from pdanet_amd import build, _lib
    build.build()
    lib = _lib.load()
    for name in ("pda_voxel_pool_scratch_doubles", "pda_voxel_pool_moments", "pda_voxel_pool_fwd", "pda_voxel_pool_bwd"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES


@pytest.mark.parametrize("batch_stats", [True, False])
def test_moment_form_equals_float64_autograd(batch_stats):
    """moment_finish / moment_backward from the nine sums and the winner sums, against autograd through BatchNorm over all
    M * ns slots with a gather at a random winner; padded duplicates and 20 % empty (all-zero) rows included."""
    from pdanet_amd.voxel_pool_modules import moment_backward, moment_finish
    g = torch.Generator().manual_seed(3)
    M, ns, C, eps = 200, 16, 32, 1e-5
    x = torch.randn(M, ns, 3, generator=g, dtype=torch.float64)
    x[:, 5:] = x[:, :1]                                                           # padded duplicates
    x[torch.rand(M, generator=g) < 0.2] = 0                                       # empty rows
    w = torch.randn(C, 3, generator=g, dtype=torch.float64, requires_grad=True)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    run_mean, run_var = torch.randn(C, generator=g, dtype=torch.float64) * 0.1, torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    arg = torch.randint(0, ns, (M, C), generator=g)
    grad = torch.randn(M, C, generator=g, dtype=torch.float64)
    y = (x @ w.t()).reshape(-1, C)
    mean, var = (y.mean(0), y.var(0, unbiased=False)) if batch_stats else (run_mean, run_var)
    z = ((y - mean) / torch.sqrt(var + eps) * gamma + beta).view(M, ns, C)
    (torch.gather(z, 1, arg[:, None, :])[:, 0] * grad).sum().backward()

    flat = x.reshape(-1, 3)
    sums = torch.cat([flat.sum(0), torch.stack([(flat[:, i] * flat[:, j]).sum() for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])])
    xs = torch.gather(x[:, :, None, :].expand(M, ns, C, 3), 1, arg[:, None, :, None].expand(M, 1, C, 3))[:, 0]     # (M, C, 3)
    wd = w.detach()
    win = torch.cat([grad.sum(0)[None], (grad * (xs * wd[None]).sum(-1)).sum(0)[None], (grad[..., None] * xs).sum(0).t()])
    n = M * ns
    m2, v2 = moment_finish(sums, n, wd)
    if batch_stats:
        assert torch.allclose(m2, mean.detach(), rtol=0, atol=1e-13) and torch.allclose(v2, var.detach(), rtol=1e-12, atol=1e-13)
    else:
        m2, v2 = run_mean, run_var
    dw, dgamma, dbeta = moment_backward(win, sums, n, wd, gamma.detach(), m2, v2, eps, batch_stats)
    for name, a, r in (("dW", dw, w.grad), ("dgamma", dgamma, gamma.grad), ("dbeta", dbeta, beta.grad)):
        err = float((a - r).abs().max())
        print("moment form, batch_stats=%s, %s: max abs error %.2e" % (batch_stats, name, err))
        assert err <= 1e-11 * max(1.0, float(r.abs().max())), name


def test_voxel_helpers_match_their_definitions():
    from pdanet_amd.spconv_utils import SparseConvTensor
    from pdanet_amd.voxel_utils import generate_voxel2pinds, get_voxel_centers
    ind = torch.tensor([[0, 1, 2, 3], [1, 0, 0, 0], [0, 3, 1, 2]], dtype=torch.int32)
    c = get_voxel_centers(ind[:, 1:4], 2, VOXEL, PCR)
    assert c.dtype == torch.float32 and torch.equal(c[0], torch.tensor([3.5 * 0.5 + 0.0, 2.5 * 0.5 - 4.0, 1.5 * 0.5 - 2.0]))
    v2p = generate_voxel2pinds(SparseConvTensor(torch.zeros(3, 4), ind, [4, 3, 5], 2))
    assert v2p.shape == (2, 4, 3, 5) and v2p.dtype == torch.int32 and int((v2p >= 0).sum()) == 3
    assert int(v2p[0, 1, 2, 3]) == 0 and int(v2p[1, 0, 0, 0]) == 1 and int(v2p[0, 3, 1, 2]) == 2 and int(v2p[1, 3, 2, 4]) == -1


# ---- the float64 restatement ----------------------------------------------------------------------------------------------
def dense_pool(layer, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices):
    """NeighborVoxelSAModuleMSG.forward on the CPU in the dtype of `layer`: the numpy voxel query, torch indexing."""
    dtype = features.dtype
    zyx = np.ascontiguousarray(new_coords[:, [0, 3, 2, 1]].numpy().astype(np.int32))
    M = zyx.shape[0]
    _, Z, Y, X = voxel2point_indices.shape
    outs = []
    for k, grouper in enumerate(layer.groupers):
        fin = layer.mlps_in[k](features.t().unsqueeze(0)).squeeze(0).t()                           # (N, C)
        idx = np.zeros((M, grouper.nsample), np.int32)
        rs.voxel_query(M, Z, Y, X, grouper.nsample, grouper.radius, *grouper.max_range, new_xyz.float().numpy(), xyz.numpy(), zyx,
                       voxel2point_indices.numpy(), idx)
        empty = torch.from_numpy(idx[:, 0] < 0)
        rows = torch.from_numpy(np.where(idx[:, :1] < 0, 0, idx)).long()
        rel = (xyz[rows] - new_xyz.float()[:, None, :]).masked_fill(empty[:, None, None], 0).to(dtype)     # the float32 difference
        f = fin[rows].masked_fill(empty[:, None, None], 0)                                         # (M, ns, C)
        pos = layer.mlps_pos[k](rel.permute(2, 0, 1).unsqueeze(0))                                 # (1, C, M, ns)
        v = torch.relu(f.permute(2, 0, 1).unsqueeze(0) + pos)
        pooled = v.max(dim=-1)[0] if layer.pool_method == 'max_pool' else v.mean(dim=-1)
        outs.append(layer.mlps_out[k](pooled).squeeze(0).t())
    return torch.cat(outs, dim=1)


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


def pool_module(npz):
    from pdanet_amd.voxel_pool_modules import NeighborVoxelSAModuleMSG
    mod = NeighborVoxelSAModuleMSG(query_ranges=[[2, 2, 2], [1, 1, 1]], radii=[1.25, 0.75], nsamples=[16, 4],
                                   mlps=[[16, 32, 32], [16, 64, 32]], pool_method='max_pool')
    mod.load_state_dict({k[len("pool_sd."):]: torch.from_numpy(v) for k, v in npz.items() if k.startswith("pool_sd.")}, strict=True)
    return mod


def pool_args(npz, device):
    t = lambda k: torch.from_numpy(npz[k]).to(device)
    return dict(xyz=t("pool_xyz"), xyz_batch_cnt=t("pool_xyz_cnt"), new_xyz=t("pool_new_xyz"), new_xyz_batch_cnt=t("pool_new_cnt"),
                new_coords=t("pool_new_coords"), voxel2point_indices=t("pool_v2p"))


def train_step(mod, forward, features, grad_out):
    f = features.clone().requires_grad_(True)
    out = forward(features=f)
    (out * grad_out).sum().backward()
    grads = {k: p.grad.detach().cpu().numpy() for k, p in mod.named_parameters()}
    stats = {k: v.detach().cpu().numpy() for k, v in mod.named_buffers() if 'running' in k}
    return out.detach(), f.grad.detach(), grads, stats


def pos_stats(stats):
    """the running statistics of the position BatchNorm, the ones the fused path computes itself"""
    return {k: v for k, v in stats.items() if k.startswith('mlps_pos.')}


# The statistics torch's own BatchNorm launches leave on the device (mlps_in, mlps_out, and mlps_pos on the composed path) are
# not this project's arithmetic and the 4x rule does not bind them: the CPU accumulates them in float64.  A float32 sum of n
# terms in any order is within (n - 1) 2^-24 of the exact sum relative to the sum of magnitudes; a batch mean and a batch
# variance are two such sums and the momentum update adds three roundings.  n = 300 x 16 slots is the most any layer here sees.
TORCH_STATS_BOUND = (2 * 300 * 16 + 3) * 2.0 ** -24


@pytest.fixture(scope="module")
def pool_truth(npz):
    """The float64 restatement of the pooling module, once: eval output, train output, gradients, running statistics."""
    mod = pool_module(npz).double()
    args = pool_args(npz, "cpu")
    feat, grad_out = torch.from_numpy(npz["pool_features"]).double(), torch.from_numpy(npz["pool_grad_out"]).double()
    mod.eval()
    with torch.no_grad():
        out_eval = dense_pool(mod, features=feat, **args)
    mod.train()
    out, gf, grads, stats = train_step(mod, functools.partial(dense_pool, mod, **args), feat, grad_out)
    gold_grads = {k[len("pool_grad."):]: v for k, v in npz.items() if k.startswith("pool_grad.")}
    gold_stats = {k[len("pool_after."):]: v for k, v in npz.items() if k.startswith("pool_after.") and 'running' in k}
    return dict(out_eval=out_eval, out=out, grad_features=gf, grads=grads, stats=stats,
                e_gold=dict(out_eval=rel(npz["pool_out_eval"], out_eval), out=rel(npz["pool_out_train"], out),
                            grad_features=rel(npz["pool_grad_features"], gf), grads=together(gold_grads, grads),
                            stats=together(gold_stats, stats), pos_stats=together(pos_stats(gold_stats), pos_stats(stats))))


def test_restatement_agrees_with_the_reference_run(pool_truth):
    """The fixture is the reference's own float32 run; the float64 restatement must be the same function."""
    for k, e in pool_truth['e_gold'].items():
        print("reference in float32 against the float64 restatement, %s: %.3e" % (k, e))
        assert e < 2e-4, k


# ---- on the GPU -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("path", ["fused", "composed"])
def test_gpu_pool_module_against_the_reference(npz, pool_truth, path, monkeypatch):
    from pdanet_amd import voxel_pool_modules as vpm
    monkeypatch.setenv(vpm.ENV, path)
    mod = pool_module(npz).cuda()
    assert mod.is_fused(0) == mod.is_fused(1) == (path == "fused")
    args = pool_args(npz, "cuda")
    feat, grad_out = torch.from_numpy(npz["pool_features"]).cuda(), torch.from_numpy(npz["pool_grad_out"]).cuda()
    gold = pool_truth['e_gold']
    mod.eval()
    with torch.no_grad():
        check(path + " eval output", rel(mod(features=feat, **args), pool_truth['out_eval']), gold['out_eval'])
    mod.train()
    out, gf, grads, stats = train_step(mod, functools.partial(mod, **args), feat, grad_out)
    check(path + " train output", rel(out, pool_truth['out']), gold['out'])
    check(path + " feature gradient", rel(gf, pool_truth['grad_features']), gold['grad_features'])
    check(path + " parameter gradients", together(grads, pool_truth['grads']), gold['grads'])
    e_stats = together(stats, pool_truth['stats'])
    print("%s running statistics, all BatchNorms: device %.3e, float32 summation bound %.3e" % (path, e_stats, TORCH_STATS_BOUND))
    assert e_stats <= TORCH_STATS_BOUND
    if path == "fused":
        check("fused running statistics of the position BatchNorm", together(pos_stats(stats), pos_stats(pool_truth['stats'])),
              gold['pos_stats'])
    assert all(int(v) == 1 for k, v in mod.named_buffers() if k.endswith('num_batches_tracked'))


@gpu
def test_gpu_fused_equals_composed(npz, pool_truth, monkeypatch):
    from pdanet_amd import voxel_pool_modules as vpm
    args = pool_args(npz, "cuda")
    feat, grad_out = torch.from_numpy(npz["pool_features"]).cuda(), torch.from_numpy(npz["pool_grad_out"]).cuda()
    res = {}
    for path in ("fused", "composed"):
        monkeypatch.setenv(vpm.ENV, path)
        mod = pool_module(npz).cuda().train()
        res[path] = train_step(mod, functools.partial(mod, **args), feat, grad_out)
    gold = pool_truth['e_gold']
    (out_f, gf_f, grads_f, stats_f), (out_c, gf_c, grads_c, stats_c) = res["fused"], res["composed"]
    check("fused against composed, output", rel(out_f, out_c), gold['out'])
    check("fused against composed, feature gradient", rel(gf_f, gf_c), gold['grad_features'])
    check("fused against composed, parameter gradients", together(grads_f, grads_c), gold['grads'])
    e_stats = together(stats_f, stats_c)
    print("fused against composed, running statistics: %.3e, float32 summation bound %.3e" % (e_stats, TORCH_STATS_BOUND))
    assert e_stats <= TORCH_STATS_BOUND
    monkeypatch.setenv(vpm.ENV, "neither")
    with pytest.raises(ValueError):
        mod(features=feat, **args)


def make_head(npz):
    from pdanet_amd.voxelrcnn_head import VoxelRCNNHead
    cfg = json.loads(str(npz["head_cfg"]))
    head = VoxelRCNNHead(BACKBONE_CHANNELS, to_attr(cfg), PCR, VOXEL, 1)
    head.load_state_dict({k[len("head_sd."):]: torch.from_numpy(v) for k, v in npz.items() if k.startswith("head_sd.")}, strict=True)
    return head


def head_batch(npz, device, dtype):
    from pdanet_amd.spconv_utils import SparseConvTensor
    feats = {}
    for name in ("x_conv2", "x_conv3"):
        feats[name] = SparseConvTensor(torch.from_numpy(npz["head_%s_features" % name]).to(device=device, dtype=dtype),
                                       torch.from_numpy(npz["head_%s_indices" % name]).to(device),
                                       npz["head_%s_spatial_shape" % name].tolist(), 2)
    rois = torch.from_numpy(npz["head_rois"]).to(device=device, dtype=dtype)      # on the 1/8 lattice: exact in either type
    return {'batch_size': 2, 'rois': rois, 'roi_scores': torch.zeros(rois.shape[:2], device=device),
            'roi_labels': torch.ones(rois.shape[:2], dtype=torch.long, device=device), 'multi_scale_3d_features': feats,
            'multi_scale_3d_strides': {'x_conv2': 2, 'x_conv3': 4}}


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
        shared = head.shared_fc_layer(pooled.view(pooled.size(0), -1))
        res['pooled_train'] = pooled
        res['rcnn_cls_train'] = head.cls_pred_layer(head.cls_fc_layers(shared))
        res['rcnn_reg_train'] = head.reg_pred_layer(head.reg_fc_layers(shared))
    return res


@gpu
def test_gpu_head_against_the_reference(npz):
    truth_head = make_head(npz).double()
    for layer in truth_head.roi_grid_pool_layers:
        layer.forward = functools.partial(dense_pool, layer)
    truth = head_outputs(truth_head, npz, "cpu", torch.float64)
    got = head_outputs(make_head(npz).cuda(), npz, "cuda", torch.float32)
    assert got['pooled_train'].shape == (12, 64, 16) and got['batch_box_preds'].shape == (2, 6, 7)
    for k in ('pooled_eval', 'batch_cls_preds', 'batch_box_preds', 'pooled_train', 'rcnn_cls_train', 'rcnn_reg_train'):
        check("head " + k, rel(got[k], truth[k]), rel(npz["head_" + k], truth[k]))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@gpu
def test_gpu_voxel_rcnn_train_and_eval():
    from pdanet_amd import model_nms_utils
    from pdanet_amd.voxel_rcnn import VoxelRCNN
    from pdanet_amd.voxel_utils import VoxelGenerator, collate_voxels
    ds = CFG['dataset']
    B = 2
    torch.manual_seed(3)
    model = VoxelRCNN(to_attr(CFG['MODEL']), 3, ds).cuda()
    rng = np.random.default_rng(5)
    pcr = np.array(ds['point_cloud_range'], np.float64)
    counts = [1500, 900]
    pts = np.concatenate([np.concatenate([rng.uniform(pcr[:3], pcr[3:], (n, 3)), rng.random((n, 1))], axis=1) for n in counts])
    offs = torch.tensor([0, counts[0], sum(counts)], dtype=torch.int64).cuda()
    gen = VoxelGenerator(ds['voxel_size'], ds['point_cloud_range'], 4, 5, 2000)
    voxels_, coords, num_points = collate_voxels(*gen.generate_batch((dev(pts.astype(np.float32)), offs, max(counts))))
    gt = np.zeros((B, 3, 8), np.float32)
    gt[0, 0] = [0.4, 0.0, -1.0, 3.9, 1.6, 1.56, 0.3, 1]
    gt[0, 1] = [0.3, 0.1, -0.6, 0.8, 0.6, 1.73, 1.2, 2]
    gt[1, 0] = [0.5, -0.1, -0.6, 1.76, 0.6, 1.73, -0.4, 3]
    roi_cfg = CFG['MODEL']['ROI_HEAD']
    n_rois, per_image = roi_cfg['NMS_CONFIG']['TRAIN']['NMS_POST_MAXSIZE'], roi_cfg['TARGET_CONFIG']['ROI_PER_IMAGE']
    # explicit draws, valid whatever the counts: the identity permutation of the foreground list, easy-background picks among
    # the zero-padded RoI rows (all but the 8 anchors' rows), hard-background pick 0
    draws = {'perm': [np.arange(n_rois)] * B, 'fg_rand': rng.random((B, per_image)), 'hard_draw': np.zeros((B, per_image), np.int64),
             'easy_draw': rng.integers(0, n_rois - 16, (B, per_image))}
    batch = {'voxels': voxels_, 'voxel_coords': coords, 'voxel_num_points': num_points, 'gt_boxes': dev(gt), 'batch_size': B}
    model.train()
    ret, tb, disp = model(dict(batch, roi_target_draws=draws))
    assert torch.isfinite(ret['loss']) and disp == {}
    assert set(tb) == {'loss_rpn', 'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir', 'rpn_loss', 'rcnn_loss_cls', 'rcnn_loss_reg',
                       'rcnn_loss_corner', 'rcnn_loss'}
    assert float(ret['loss'].detach()) == pytest.approx(float(tb['loss_rpn'] + tb['rcnn_loss']), rel=1e-5)
    assert model.roi_head.forward_ret_dict['rcnn_cls'].shape == (B * per_image, 1)
    assert int(model.roi_head.forward_ret_dict['status'].abs().sum()) == 0
    ret['loss'].backward()
    for name, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    model.eval()
    with torch.no_grad():
        pred_dicts, recall = model(dict(batch))
        assert len(pred_dicts) == B and set(pred_dicts[0]) == {'pred_boxes', 'pred_scores', 'pred_labels'}
        assert set(recall) == {'gt', 'roi_0.3', 'rcnn_0.3', 'roi_0.5', 'rcnn_0.5', 'roi_0.7', 'rcnn_0.7'}
        # the labels are the first stage's: one score column, so the argmax would say 1 everywhere
        bd = dict(batch)
        for module in model.module_list:
            bd = module(bd)
        assert bd['has_class_labels'] and bd['batch_cls_preds'].shape[-1] == 1
        bd['roi_labels'] = torch.full_like(bd['roi_labels'], 3)
        padded = model_nms_utils.post_processing(bd, model.model_cfg['POST_PROCESSING'], 3)
        valid = torch.arange(padded['pred_labels'].shape[1], device='cuda')[None, :] < padded['num_pred'][:, None]
        assert int(valid.sum()) > 0 and bool((padded['pred_labels'][valid] == 3).all()) and not padded['pred_labels'][~valid].any()
