"""This repo's model code against golden tensors produced by the REFERENCE's own Python
composition (tests/golden/make_golden.py: reference pointnet2_utils / pointnet2_modules /
IASSD_backbone on CPU, extension stubbed with the oracle).  Weights are not stored: both sides
fill them by state-dict key (tests/golden/detweights.py), which also proves the key schema.

CPU part: state-dict schema, pure-torch sub-blocks.  GPU part (-m gpu): everything that goes
through the HIP operators.  Tolerance: indices exact; features 1e-4 absolute on O(1) values
(fp32 CPU GEMM vs rocBLAS accumulate in different orders)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from detweights import fill_deterministic  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "reference_composition.npz"))
META = json.load(open(os.path.join(HERE, "golden", "reference_composition_meta.json")))
SCHEMA = json.load(open(os.path.join(HERE, "golden", "backbone_state_dict_schema.json")))


def T(name, device="cpu"):
    return torch.from_numpy(G[name]).to(device)


def close(a, ref, atol=1e-4, rtol=1e-4):
    np.testing.assert_allclose(a.detach().cpu().numpy(), ref, atol=atol, rtol=rtol)


def close_dense(a, ref, frac=0.98, tight=1e-4, atol=2e-3, rtol=1e-2):
    """Outputs that went through several fp32 GEMM + batch-stat BatchNorm + softmax stages:
    rocBLAS and the CPU BLAS accumulate in different orders, and a few elements next to a ReLU /
    small-variance BN channel move by ~1e-3.  Require `frac` of the elements within `tight`
    and every element within (atol, rtol)."""
    a = a.detach().cpu().numpy()
    err = np.abs(a - ref)
    assert (err <= tight + tight * np.abs(ref)).mean() >= frac, (err > tight + tight * np.abs(ref)).mean()
    np.testing.assert_allclose(a, ref, atol=atol, rtol=rtol)


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("tag,yaml_name", [("once", "once_pda_ssd.yaml"), ("kitti", "kitti_pda_ssd.yaml")])
def test_backbone_state_dict_schema(tag, yaml_name):
    from pdanet_amd.backbone import build_backbone
    model, _ = build_backbone(yaml_name)
    mine = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert mine == SCHEMA[tag]          # same keys, same order, same shapes
    assert sum(p.numel() for p in model.parameters()) == META[tag + "_params"]


def test_transformer_block_cpu():
    from pdanet_amd.pointnet2_modules import TransformerEncoderLayerPreNorm
    tr = fill_deterministic(TransformerEncoderLayerPreNorm(d_model=32, nhead=4, dim_feedforward=16, dropout=0.0)).eval()
    close(tr(T("transformer_in")), G["transformer_out"], atol=2e-5)


def test_density_net_cpu():
    from pdanet_amd.pointnet2_modules import PointConvDensitySetAbstraction
    dn = fill_deterministic(PointConvDensitySetAbstraction(0.8))
    dn.eval(); close(dn(T("density_in")), G["density_out_eval"], atol=2e-5)
    dn.train(); close(dn(T("density_in")), G["density_out_train"], atol=2e-5)


def test_vote_layer_cpu():
    from pdanet_amd.pointnet2_modules import Vote_layer
    vote = fill_deterministic(Vote_layer(mlp_list=[16], pre_channel=8, max_translate_range=[3.0, 3.0, 2.0])).eval()
    v = vote(T("vote_xyz_in"), T("vote_feat_in"))
    close(v[0], G["vote_xyz"], atol=2e-5); close(v[3], G["vote_offsets"], atol=2e-5)
    assert v[1].shape[-1] == 0 and v[2] is not None


# ------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


def _sa_layer(cls_name, mlps, **override):
    from pdanet_amd import pointnet2_modules as pm
    kw = dict(META["sa_kwargs"]); kw.update(override)
    return fill_deterministic(getattr(pm, cls_name)(mlps=[list(m) for m in mlps], **kw)).cuda()


@gpu
@pytest.mark.parametrize("name,cls_name,mlp_key,feat_key", [
    ("sa", "PointnetSAModuleMSG_WithSampling", "sa_mlps", "sa_feats"),
    ("pda", "PointnetSAModuleMSG_WithSampling_Ellipsoid", "pda_mlps", "pda_feats")])
def test_sa_layers_vs_reference_composition(name, cls_name, mlp_key, feat_key):
    xyz, feats = T("sa_xyz", "cuda"), T(feat_key, "cuda")
    layer = _sa_layer(cls_name, META[mlp_key])
    for mode in ["eval", "train"]:
        layer.train(mode == "train")
        with torch.no_grad():
            nx, nf, cf, sidx = layer(xyz, feats, None)
        assert np.array_equal(sidx.cpu().numpy(), G["%s_%s_idx" % (name, mode)])      # D-FPS indices exact
        assert np.array_equal(nx.cpu().numpy(), G["%s_%s_new_xyz" % (name, mode)])    # gathered coords exact
        (close if name == "sa" else close_dense)(nf, G["%s_%s_new_features" % (name, mode)])
        (close if name == "sa" else close_dense)(cf, G["%s_%s_cls" % (name, mode)])
    layer2 = _sa_layer(cls_name, META[mlp_key], sample_type_list=["ctr_aware"]).eval()
    with torch.no_grad():
        nx, nf, cf, sidx = layer2(xyz, feats, T("sa_cls", "cuda"))
    # torch.topk tie order is unspecified: compare the sampled SETS, then features row-matched
    ref_idx = G["%s_ctr_idx" % name]
    got_idx = sidx.cpu().numpy()
    for b in range(ref_idx.shape[0]):
        assert set(ref_idx[b].tolist()) == set(got_idx[b].tolist())
    # the sets are equal and top-k indices are distinct: the permutation that takes got_idx[b] to ref_idx[b], applied to the
    # centre axis of nf (B, C, npoint) -- the features are compared whatever order the ties came out in
    rows = []
    for b in range(ref_idx.shape[0]):
        order = np.argsort(got_idx[b], kind="stable")
        perm = order[np.searchsorted(got_idx[b][order], ref_idx[b])]
        assert np.array_equal(got_idx[b][perm], ref_idx[b])
        rows.append(nf[b].index_select(-1, torch.from_numpy(perm).to(nf.device)))
    (close if name == "sa" else close_dense)(torch.stack(rows), G["%s_ctr_new_features" % name])


@gpu
def test_sa_layer_with_given_centres():
    layer = _sa_layer("PointnetSAModuleMSG_WithSampling", META["sa_mlps"]).eval()
    with torch.no_grad():
        nx, nf, cf, sidx = layer(T("sa_xyz", "cuda"), T("sa_feats", "cuda"), None, ctr_xyz=T("sa_ctrxyz_in", "cuda"))
    close(nf, G["sa_ctrxyz_new_features"])


@gpu
def test_groupers_vs_reference_composition():
    from pdanet_amd import pointnet2_utils as pu
    xyz, feats, ctr = T("sa_xyz", "cuda"), T("sa_feats", "cuda"), T("sa_ctrxyz_in", "cuda")
    close(pu.QueryAndGroup(2.0, 8)(xyz, ctr, feats), G["grouper_vanilla"], atol=1e-5)
    close(pu.QueryAndGroup_alone_grouped_density_directional(2.0, 8)(xyz, ctr, feats), G["grouper_pda"], atol=1e-5)


@gpu
def test_fp_module_vs_reference_composition():
    from pdanet_amd.pointnet2_modules import PointnetFPModule
    fp = fill_deterministic(PointnetFPModule(mlp=[10, 16])).cuda().eval()
    xyz = T("sa_xyz", "cuda")
    with torch.no_grad():
        out = fp(xyz, xyz[:, :100].contiguous(), T("fp_unknown_feats", "cuda"), T("fp_known_feats", "cuda"))
    close(out, G["fp_out"])      # north_star: interpolated features within 1e-4


@pytest.fixture(scope="module", params=["eval", "train"])
def backbone_forward(request):
    """(mode, batch_dict) of one backbone forward on the golden scene, shared by the two tests below."""
    from pdanet_amd import synth, config
    from pdanet_amd.backbone import IASSD_Backbone
    mode = request.param
    cfg = config.load_yaml("once_pda_ssd.yaml")
    cfg.MODEL.BACKBONE_3D.SA_CONFIG.NPOINT_LIST = META["backbone_npoint_list"]
    model = fill_deterministic(IASSD_Backbone(cfg.MODEL.BACKBONE_3D, num_class=5, input_channels=4)).cuda()
    model.train(mode == "train")
    pts = torch.from_numpy(synth.batch_points(2, 2048, config_id=91, dist="L")).cuda()
    with torch.no_grad():
        bd = model({"batch_size": 2, "points": pts})
    return mode, bd


def _xyz_rows(a):
    return [tuple(r) for r in a.round(4).tolist()]


@gpu
def test_backbone_vs_reference_composition(backbone_forward):
    mode, bd = backbone_forward
    # layer 1 samples with D-FPS: coordinates are gathered, so they must match bit for bit
    assert np.array_equal(bd["encoder_xyz"][1].cpu().numpy(), G["bb_%s_encoder_xyz_1" % mode])
    assert np.array_equal(bd["encoder_xyz"][2].cpu().numpy(), G["bb_%s_encoder_xyz_2" % mode])
    close(bd["encoder_features"][1][:, :8, :16], G["bb_%s_feat_1_slice" % mode], atol=2e-4, rtol=1e-3)
    close(bd["encoder_features"][2][:, :8, :16], G["bb_%s_feat_2_slice" % mode], atol=2e-4, rtol=1e-3)
    close(bd["sa_ins_preds"][1], G["bb_%s_sa_ins_preds_1" % mode], atol=5e-4, rtol=1e-3)
    # layers 2-3 sample by top-k of predicted scores: same SET of centres (order/near-ties may differ)
    for li in (3, 4):
        ref = G["bb_%s_encoder_xyz_%d" % (mode, li)]
        got = bd["encoder_xyz"][li].cpu().numpy()
        for b in range(ref.shape[0]):
            a = {tuple(r) for r in ref[b].round(4).tolist()}
            c = {tuple(r) for r in got[b].round(4).tolist()}
            assert len(a & c) >= 0.98 * len(a), (li, len(a & c), len(a))
    for li in range(1, 7):
        if li == 5:
            continue  # vote layer's "features" are empty
        ref = float(G["bb_%s_feat_%d_absmean" % (mode, li)][0])
        got = float(bd["encoder_features"][li].abs().mean())
        assert abs(got - ref) <= 2e-3 * max(1.0, abs(ref)), (li, got, ref)


@gpu
def test_backbone_heads_vs_reference_composition(backbone_forward):
    """centers, ctr_offsets and centers_features behind the top-k layers.  Where the layer-3 and layer-4 centre sets equal
    the golden's, the rows are matched by their layer-4 coordinates and compared whatever order the top-k left them in;
    where a set differs (a near-tie of two scores went the other way: other centres, other rows) the test is SKIPPED with
    the overlap counts, so that the report shows that nothing was compared."""
    mode, bd = backbone_forward
    overlap = []
    for li in (3, 4):
        ref = G["bb_%s_encoder_xyz_%d" % (mode, li)]
        got = bd["encoder_xyz"][li].cpu().numpy()
        for b in range(ref.shape[0]):
            a, c = set(_xyz_rows(ref[b])), set(_xyz_rows(got[b]))
            overlap.append((li, b, len(a & c), len(a), a == c))
    if not all(o[4] for o in overlap):
        pytest.skip("%s: centre sets differ from the golden's, (layer, scene, common, of): %s"
                    % (mode, [o[:4] for o in overlap if not o[4]]))
    ref4, got4 = G["bb_%s_encoder_xyz_4" % mode], bd["encoder_xyz"][4].cpu().numpy()
    n = ref4.shape[1]
    perm = []
    for b in range(ref4.shape[0]):
        where = {r: i for i, r in enumerate(_xyz_rows(got4[b]))}
        assert len(where) == n
        perm += [b * n + where[r] for r in _xyz_rows(ref4[b])]
    perm = torch.tensor(perm, dtype=torch.long, device=bd["centers"].device)
    close(bd["centers"][perm], G["bb_%s_centers" % mode], atol=1e-3, rtol=1e-3)
    close(bd["ctr_offsets"][perm], G["bb_%s_ctr_offsets" % mode], atol=1e-3, rtol=1e-3)
    close(bd["centers_features"][perm], G["bb_%s_centers_features" % mode], atol=2e-3, rtol=2e-3)


@gpu
@pytest.mark.parametrize("cls_name,mlp_key,feat_key", [
    ("PointnetSAModuleMSG_WithSampling", "sa_mlps", "sa_feats"),
    ("PointnetSAModuleMSG_WithSampling_Ellipsoid", "pda_mlps", "pda_feats")])
def test_channels_last_path_equals_channel_major_path(cls_name, mlp_key, feat_key):
    """The point-major execution (CHANNELS_LAST) against the reference-layout execution of the same
    module: forward outputs and gradients w.r.t. inputs and parameters, train-mode BN."""
    xyz = T("sa_xyz", "cuda")
    outs = {}
    for cl in (False, True):
        layer = _sa_layer(cls_name, META[mlp_key]).train()
        layer.channels_last = cl
        feats = T(feat_key, "cuda").clone().requires_grad_(True)
        nx, nf, cf, sidx = layer(xyz, feats, None)
        (nf.pow(2).mean() + cf.pow(2).mean()).backward()
        grads = {k: p.grad.clone() for k, p in layer.named_parameters() if p.grad is not None}
        outs[cl] = (nf.detach(), cf.detach(), feats.grad.clone(), grads,
                    {k: v.clone() for k, v in layer.state_dict().items() if "running" in k})
    a, b = outs[False], outs[True]
    close_dense(b[0], a[0].cpu().numpy()); close_dense(b[1], a[1].cpu().numpy())
    scale = float(a[2].abs().max())
    assert float((a[2] - b[2]).abs().max()) <= 5e-3 * scale + 1e-7
    assert set(a[3]) == set(b[3])
    gmax = max(float(v.abs().max()) for v in a[3].values())
    for k in a[3]:
        # weights in front of a BatchNorm have mathematically ~zero gradient along their own
        # direction: their gradients are round-off sized, so the floor is relative to the largest
        # gradient of the layer
        s = float(a[3][k].abs().max())
        assert float((a[3][k] - b[3][k]).abs().max()) <= 1e-2 * s + 1e-3 * gmax, k
    for k in a[4]:   # BatchNorm running statistics updated identically
        assert torch.allclose(a[4][k], b[4][k], rtol=1e-4, atol=1e-5), k


@gpu
def test_kitti_backbone_forward_backward_runs():
    """The KITTI yaml (4096/1024/512/256 centres, layer 5 with a 1024-wide chain): forward +
    backward on a synthetic 16384-pt KITTI batch; shapes as the head expects, finite gradients."""
    from pdanet_amd import synth
    from pdanet_amd.backbone import build_backbone
    model, cfg = build_backbone("kitti_pda_ssd.yaml")
    model = fill_deterministic(model).cuda().train()
    pts = torch.from_numpy(synth.batch_points(2, 16384, config_id=3, dist="L", dataset="kitti")).cuda()
    bd = model({"batch_size": 2, "points": pts})
    assert bd["centers"].shape == (2 * 256, 4) and bd["centers_features"].shape == (2 * 256, 512)
    assert [t.shape[1] for t in bd["encoder_xyz"]] == [16384, 4096, 1024, 512, 256, 256, 256]
    assert bd["sa_ins_preds"][1].shape == (2, 1024, 1 + 3) and bd["sa_ins_preds"][2].shape == (2, 512, 1 + 3)
    loss = bd["centers_features"].pow(2).mean() + bd["ctr_offsets"][:, 1:].pow(2).mean()
    loss.backward()
    n_grad = sum(1 for p in model.parameters() if p.grad is not None)
    assert n_grad >= 0.9 * sum(1 for _ in model.parameters())
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


@gpu
def test_inference_forward_captures_into_hipgraph():
    """The whole backbone inference forward (side-stream D-FPS prefetch, fused SA kernels, point-
    major PDA layers) is capturable: no allocation/synchronisation/host copies in the C ABI or the
    model code.  Replay must reproduce the eager result bit for bit."""
    from pdanet_amd import synth, fused_ops, pointnet2_utils as pu
    from pdanet_amd.backbone import build_backbone
    model, _ = build_backbone("once_pda_ssd.yaml")
    model = fill_deterministic(model).cuda().eval()
    fused_ops.enable_fused(model)
    pts = torch.from_numpy(synth.batch_points(2, 4096, config_id=8)).cuda()
    with torch.no_grad():
        ragged = model({"batch_size": 2, "points": pts})["centers_features"].clone()
        # under capture the PDA encoder runs in its dense form (the unique-token form reads a token count on the
        # host, pointnet2_utils.ragged_plans): the bit-for-bit reference is the eager dense form
        pu.RAGGED_TOKENS = False
        try:
            for _ in range(2):
                ref = model({"batch_size": 2, "points": pts})["centers_features"].clone()
        finally:
            pu.RAGGED_TOKENS = True
    # same result up to fp32 re-association -- except where a 1e-6 score difference flips the top-k centre choice of
    # layers 2-3 (random-init scores are nearly equal), which replaces whole rows: compare the bulk
    agree = ((ragged - ref).abs() <= 2e-4 * max(1.0, ref.abs().max().item())).float().mean().item()
    assert agree > 0.97, agree
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out = model({"batch_size": 2, "points": pts})["centers_features"]
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


@pytest.mark.gpu
def test_resident_input_prefetch_gives_identical_results():
    """batch_dict['inputs_resident'] only changes WHEN the coordinate-only sampling may start (no wait for the
    current stream), never what it computes."""
    import torch
    from pdanet_amd import synth
    from pdanet_amd.backbone import build_backbone
    torch.manual_seed(1)
    model, _ = build_backbone("once_pda_ssd.yaml")
    model = model.cuda().eval()
    pts = torch.from_numpy(synth.batch_points(2, 4096, config_id=2)).cuda()
    torch.cuda.synchronize()
    outs = []
    for resident in (False, True, True):
        with torch.no_grad():
            bd = model({'batch_size': 2, 'points': pts, 'inputs_resident': resident})
        outs.append((bd['centers'].clone(), bd['centers_features'].clone(), bd['encoder_xyz'][2].clone()))
    torch.cuda.synchronize()
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_backbone_prefetch_starts_the_next_forward_early_and_changes_nothing():
    """backbone.prefetch(points): sampling, layer-1 ball queries and unique-token plans of the NEXT forward, started on the
    side stream ahead of time.  Same results as a plain forward; a stash made for another tensor is ignored."""
    import torch
    from pdanet_amd import synth
    from pdanet_amd.backbone import build_backbone
    torch.manual_seed(1)
    model, _ = build_backbone("once_pda_ssd.yaml")
    model = model.cuda().eval()
    pts = torch.from_numpy(synth.batch_points(2, 4096, config_id=2)).cuda()
    other = torch.from_numpy(synth.batch_points(2, 4096, config_id=7)).cuda()
    torch.cuda.synchronize()

    def run(p):
        with torch.no_grad():
            bd = model({'batch_size': 2, 'points': p, 'inputs_resident': True})
        return bd['centers'].clone(), bd['centers_features'].clone(), bd['encoder_xyz'][2].clone()
    ref, ref_other = run(pts), run(other)
    model.prefetch(pts, 2)
    assert len(model._prefetched) == 1
    got = run(pts)                               # consumes the stash
    assert len(model._prefetched) == 0
    model.prefetch(pts, 2)
    got_other = run(other)                       # stash belongs to another batch: dropped, computed afresh
    assert len(model._prefetched) == 0
    # two batches in flight (a serving loop prefetches batch i + 1 BEFORE the forward of batch i): consumed oldest first
    model.prefetch(pts, 2)
    model.prefetch(other, 2)
    a1, a2 = run(pts), run(other)
    assert len(model._prefetched) == 0
    for a, b in zip(ref + ref_other, a1 + a2):
        assert torch.equal(a, b)
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
    for a, b in zip(ref_other, got_other):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_inference_graph_tail_equals_eager_forward():
    """IASSD_Backbone.graph_tail_infer (eval, no_grad: the layers behind the last token-count read replayed as one hipGraph)
    against the launch-by-launch forward: every output bit for bit, over three different batches (the graph's buffers are
    refilled), and again after the weights changed (a new capture).  Third round: once that round's graph is captured, the
    running means of the last layer's BatchNorms move in place (no parameter, no epoch does): a new capture again."""
    from pdanet_amd import fused_ops, synth
    from pdanet_amd.backbone import build_backbone
    torch.manual_seed(3)
    model, _ = build_backbone("once_pda_ssd.yaml")
    model = model.cuda().eval()
    fused_ops.enable_fused(model)
    B, N = 2, 16384
    keys = ("centers_features", "centers", "centers_origin", "ctr_offsets")

    def fwd(pts, graphed):
        model.graph_tail_infer = graphed
        with torch.no_grad():
            bd = model({'batch_size': B, 'points': pts})
        out = {k: bd[k].clone() for k in keys}
        out.update({"xyz%d" % i: t.clone() for i, t in enumerate(bd['encoder_xyz'])})
        out.update({"f%d" % i: t.clone() for i, t in enumerate(bd['encoder_features']) if t is not None})
        out.update({"c%d" % i: t.clone() for i, t in enumerate(bd['encoder_coords'])})
        out.update({"p%d" % i: t.clone() for i, t in enumerate(bd['sa_ins_preds']) if torch.is_tensor(t)})
        return out
    for rnd in range(3):
        for seed in (2, 12, 22):
            if rnd == 2 and seed == 12:             # after the weight change of round 1 and the capture for it (seed 2)
                with torch.no_grad():
                    for m in model.SA_modules[5].modules():
                        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                            m.running_mean.add_(0.1)
            pts = torch.from_numpy(synth.batch_points(B, N, config_id=seed, dist="L")).cuda()
            a, b = fwd(pts, True), fwd(pts, False)
            assert set(a) == set(b)
            for k in b:
                assert torch.equal(a[k], b[k]), (rnd, seed, k)
        with torch.no_grad():                       # new weights: the captured graph must not be replayed with the old ones
            for p in model.SA_modules[5].parameters():
                p.mul_(1.01)
    assert model._tail_graph is not None
