#!/usr/bin/env python
"""Generates tests/golden/reference_composition.npz, reference_composition_meta.json and backbone_state_dict_schema.json by
running the REFERENCE's own Python composition (pcdet/ops/pointnet2/pointnet2_batch/{pointnet2_utils,pointnet2_modules,
PointFormer}.py and pcdet/models/backbones_3d/IASSD_backbone.py) on CPU, with its CUDA extension module replaced by a stub
backed by this repo's CPU oracle (reference_loader.pointnet2_batch_stub).

Run with the reference checkout:  python tests/golden/make_golden.py /path/to/reference
The reference sources are imported from where they lie; nothing of them is copied.  What is
committed is data: seeds, small inputs, and the reference composition's outputs.
"""
import json
import os
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from reference_loader import cpu_torch, load, pointnet2_batch_stub, reference_root  # noqa: E402
from detweights import fill_deterministic  # noqa: E402
from pdanet_amd.config import to_attr  # noqa: E402

BATCH = "ops.pointnet2.pointnet2_batch."


def import_reference(root):
    """-> (pointnet2_utils, PointFormer, pointnet2_modules, IASSD_backbone) of the reference, as pcdet.*"""
    cpu_torch()              # the reference allocates with torch.cuda.IntTensor/FloatTensor (pointnet2_utils.py:25-26...)
    # semantic_view.py is visualisation only; spvnas_cluster is the unused torchsparse import (IASSD_backbone.py:7)
    stubs = {BATCH + "pointnet2_batch_cuda": pointnet2_batch_stub(), BATCH + "semantic_view": {},
             "models.backbones_3d.cluster.spvnas_cluster": {"SPVNAS": object}}
    return load(root, "pcdet", [BATCH + "pointnet2_utils", BATCH + "PointFormer", BATCH + "pointnet2_modules",
                                "models.backbones_3d.IASSD_backbone"], stubs=stubs, real_paths=True)


def scene_points(b, n, seed):
    from pdanet_amd import synth
    return synth.batch_points(b, n, config_id=seed, dist="L")


def t2n(x):
    return x.detach().cpu().numpy()


def main():
    torch.set_num_threads(8)
    root = reference_root()
    pu, PF, pm, bb = import_reference(root)
    out = {}
    meta = {"generator": "tests/golden/make_golden.py", "reference": "Geo3DSmart/PDANet @ " + root,
            "torch": torch.__version__}

    # 1. state-dict schema of the reference backbone for both yamls
    schema = {}
    for tag, path in [("once", root + "/tools/cfgs/once_models/PDA-SSD.yaml"),
                      ("kitti", root + "/tools/cfgs/kitti_models/PDA-SSD.yaml")]:
        cfg = to_attr(yaml.safe_load(open(path)))
        model = bb.IASSD_Backbone(cfg.MODEL.BACKBONE_3D, num_class=len(cfg.CLASS_NAMES), input_channels=4)
        schema[tag] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
        meta[tag + "_params"] = sum(p.numel() for p in model.parameters())
    json.dump(schema, open(os.path.join(HERE, "backbone_state_dict_schema.json"), "w"))

    # 2. pure-torch sub-blocks
    torch.manual_seed(0)
    tr = fill_deterministic(PF.TransformerEncoderLayerPreNorm(d_model=32, nhead=4, dim_feedforward=16, dropout=0.0)).eval()
    x = torch.randn(8, 6, 32)
    out["transformer_in"] = t2n(x); out["transformer_out"] = t2n(tr(x))
    dn = fill_deterministic(pm.PointConvDensitySetAbstraction(0.8))
    d = torch.rand(2, 1, 5, 8) + 0.1
    dn.eval(); out["density_in"] = t2n(d); out["density_out_eval"] = t2n(dn(d))
    dn.train(); out["density_out_train"] = t2n(dn(d))
    vote = fill_deterministic(pm.Vote_layer(mlp_list=[16], pre_channel=8, max_translate_range=[3.0, 3.0, 2.0])).eval()
    vx, vf = torch.randn(2, 10, 3) * 5, torch.randn(2, 8, 10) * 3
    v = vote(vx, vf)
    out["vote_xyz_in"], out["vote_feat_in"] = t2n(vx), t2n(vf)
    out["vote_xyz"], out["vote_offsets"] = t2n(v[0]), t2n(v[3])

    # 3. one vanilla SA layer and one PDA layer through the stub extension (B=2, N=1024)
    pts = scene_points(2, 1024, seed=77)
    xyz = torch.from_numpy(pts[:, 1:4]).view(2, 1024, 3).contiguous()
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(2, 6, 1024, generator=g)
    cls_feats = torch.randn(2, 1024, 3, generator=g)
    out["sa_xyz"], out["sa_feats"], out["sa_cls"] = t2n(xyz), t2n(feats), t2n(cls_feats)
    sa_kwargs = dict(npoint_list=[256], sample_range_list=[-1], sample_type_list=["D-FPS"],
                     radii=[2.0, 6.0], nsamples=[8, 16], use_xyz=True, dilated_group=False,
                     aggregation_mlp=[24], confidence_mlp=[12], num_class=3)
    meta["sa_kwargs"] = sa_kwargs
    meta["sa_mlps"] = [[6, 8, 16], [6, 8, 12]]
    meta["pda_mlps"] = [[6, 8, 16], [6, 10, 12]]
    for name, cls, mlps in [("sa", pm.PointnetSAModuleMSG_WithSampling, meta["sa_mlps"]),
                            ("pda", pm.PointnetSAModuleMSG_WithSampling_Ellipsoid, meta["pda_mlps"])]:
        if name == "pda":
            mlps = [[8] + m[1:] for m in mlps]  # C = 8: feature channels must equal mlp_spec[0]
            meta["pda_mlps"] = mlps
            f_in = torch.randn(2, 8, 1024, generator=g)
            out["pda_feats"] = t2n(f_in)
        else:
            f_in = feats
        layer = fill_deterministic(cls(mlps=[list(m) for m in mlps], **sa_kwargs))
        for mode in ["eval", "train"]:
            layer.train(mode == "train")
            with torch.no_grad():
                nx, nf, cf, sidx = layer(xyz, f_in, None)
            out["%s_%s_new_xyz" % (name, mode)] = t2n(nx)
            out["%s_%s_new_features" % (name, mode)] = t2n(nf)
            out["%s_%s_cls" % (name, mode)] = t2n(cf)
            out["%s_%s_idx" % (name, mode)] = t2n(sidx)
        # ctr-aware sampling variant (top-k of sigmoid(max cls))
        kw = dict(sa_kwargs); kw["sample_type_list"] = ["ctr_aware"]
        layer2 = fill_deterministic(cls(mlps=[list(m) for m in mlps], **kw)).eval()
        with torch.no_grad():
            nx, nf, cf, sidx = layer2(xyz, f_in, cls_feats)
        out["%s_ctr_new_features" % name] = t2n(nf)
        out["%s_ctr_idx" % name] = t2n(sidx)
    # vanilla layer centred on given ctr_xyz (layer-5 style: centres are not points)
    ctr = xyz[:, :64].contiguous() + 0.3
    layer = fill_deterministic(pm.PointnetSAModuleMSG_WithSampling(mlps=[list(m) for m in meta["sa_mlps"]], **sa_kwargs)).eval()
    with torch.no_grad():
        nx, nf, cf, sidx = layer(xyz, feats, None, ctr_xyz=ctr)
    out["sa_ctrxyz_in"] = t2n(ctr); out["sa_ctrxyz_new_features"] = t2n(nf)

    # 4. groupers on their own
    gq = pu.QueryAndGroup(2.0, 8)(xyz, ctr, feats)
    gd = pu.QueryAndGroup_alone_grouped_density_directional(2.0, 8)(xyz, ctr, feats)
    out["grouper_vanilla"], out["grouper_pda"] = t2n(gq), t2n(gd)

    # 5. FP module (three_nn + three_interpolate composition)
    fp = fill_deterministic(pm.PointnetFPModule(mlp=[6 + 4, 16])).eval()
    known = xyz[:, :100].contiguous(); kf = torch.randn(2, 6, 100, generator=g); uf = torch.randn(2, 4, 1024, generator=g)
    with torch.no_grad():
        out["fp_out"] = t2n(fp(xyz, known, uf, kf))
    out["fp_known_feats"], out["fp_unknown_feats"] = t2n(kf), t2n(uf)

    # 6. the whole backbone, scaled-down point counts (real channel widths), eval + train BN
    cfg = to_attr(yaml.safe_load(open(root + "/tools/cfgs/once_models/PDA-SSD.yaml")))
    sa = cfg.MODEL.BACKBONE_3D.SA_CONFIG
    sa["NPOINT_LIST"] = [[2048], [512], [256], [128], [-1], [128]]
    meta["backbone_npoint_list"] = sa["NPOINT_LIST"]
    model = fill_deterministic(bb.IASSD_Backbone(cfg.MODEL.BACKBONE_3D, num_class=5, input_channels=4))
    bpts = torch.from_numpy(scene_points(2, 2048, seed=91))
    for mode in ["eval", "train"]:
        model.train(mode == "train")
        with torch.no_grad():
            bd = model({"batch_size": 2, "points": bpts.clone()})
        for k in ["centers", "centers_origin", "ctr_offsets", "centers_features"]:
            out["bb_%s_%s" % (mode, k)] = t2n(bd[k])
        for li, t in enumerate(bd["encoder_xyz"]):
            out["bb_%s_encoder_xyz_%d" % (mode, li)] = t2n(t)
        for li, t in enumerate(bd["sa_ins_preds"]):
            if not isinstance(t, list):
                out["bb_%s_sa_ins_preds_%d" % (mode, li)] = t2n(t)
        for li, t in enumerate(bd["encoder_features"][1:], start=1):
            # keep fixtures small: per-layer feature checksums + a slice
            out["bb_%s_feat_%d_slice" % (mode, li)] = t2n(t[:, :8, :16])
            out["bb_%s_feat_%d_absmean" % (mode, li)] = np.array([t.abs().mean().item()], np.float32)

    np.savez_compressed(os.path.join(HERE, "reference_composition.npz"), **out)
    json.dump(meta, open(os.path.join(HERE, "reference_composition_meta.json"), "w"), indent=1)
    print("wrote", len(out), "arrays;", sum(v.nbytes for v in out.values()) / 1e6, "MB raw")


if __name__ == "__main__":
    main()
