#!/usr/bin/env python
"""Times the sparse 3D convolutions at the KITTI SECOND shape: 4 synthetic scenes through VoxelGenerator at second.yaml's
voxel size (0.05, 0.05, 0.1 m over [0, -40, -3, 70.4, 40, 1]: a 41 x 1600 x 1408 grid, at most 16000 voxels of 5 points a
scene), MeanVFE, then the levels of VoxelBackBone8x.

One JSON line per (level, stage, variant): the median and the minimum over --reps calls, wall clock between two device
synchronisations, after --warmup calls; the variants of a stage alternate call by call, so that both see the same machine.

  index     the rulebook build of the level (device only; a strided build includes its one host read).
  forward / dgrad / wgrad
            device: pda_spconv_gemm / pda_spconv_gemm transposed / pda_spconv_wgrad.   torch: a composition from the SAME
            neighbour map on the same card, per tap index_select, mm, index_add_ -- what spconv's native algorithm does.
            The per-tap row lists of the torch variant are made outside the timed region.
  backbone  VoxelBackBone8x forward + backward (sum of squares of the output), rulebooks rebuilt every call; torch: the same
            modules with the convolution swapped for the composition (rulebooks still from the device index stage).
--only STAGE runs one stage (for a `rocprofv3 --kernel-trace --stats` run of its own).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdanet_amd import spconv_utils as sp  # noqa: E402
from pdanet_amd.config import to_attr  # noqa: E402
from pdanet_amd.mean_vfe import MeanVFE  # noqa: E402
from pdanet_amd.spconv_backbone import VoxelBackBone8x  # noqa: E402
from pdanet_amd.voxel_utils import VoxelGenerator, collate_voxels, grid_size  # noqa: E402

PCR = [0, -40, -3, 70.4, 40, 1]
VS = [0.05, 0.05, 0.1]
# name, kind, C_in, C_out, kernel, stride, padding; a strided level feeds the next levels its output sites
LEVELS = [('subm1', 'subm', 16, 16, 3, 1, 1), ('spconv2', 'spconv', 16, 32, 3, 2, 1), ('subm2', 'subm', 32, 32, 3, 1, 1),
          ('spconv3', 'spconv', 32, 64, 3, 2, 1), ('subm3', 'subm', 64, 64, 3, 1, 1),
          ('spconv4', 'spconv', 64, 64, 3, 2, (0, 1, 1)), ('subm4', 'subm', 64, 64, 3, 1, 1),
          ('spconv_down2', 'spconv', 64, 128, (3, 1, 1), (2, 1, 1), 0)]


def scenes(rng, batch, n_points):
    """A crude lidar sweep a scene: ground returns thinning with range, and a few dozen upright boxes of returns."""
    pts = []
    for _ in range(batch):
        r = np.abs(rng.standard_normal(n_points)) * 22 + 2
        az = rng.uniform(-0.72, 0.72, n_points)
        x, y = r * np.cos(az), r * np.sin(az)
        z = -1.7 + rng.standard_normal(n_points) * 0.03 + 0.002 * r
        k = n_points // 3
        cx, cy = rng.uniform(5, 60, 40), rng.uniform(-30, 30, 40)
        which = rng.integers(0, 40, k)
        x[:k], y[:k] = cx[which] + rng.uniform(-2, 2, k), cy[which] + rng.choice([-0.8, 0.8], k) + rng.standard_normal(k) * 0.02
        z[:k] = rng.uniform(-1.7, 0.2, k)
        pts.append(np.stack([x, y, z, rng.random(n_points)], axis=1).astype(np.float32))
    return pts


def tap_lists(book):
    """Per tap the (output rows, input rows) of the neighbour map, for the torch composition."""
    if getattr(book, 'taps_lists', None) is None:
        book.taps_lists = []
        for t in range(book.taps):
            o = torch.nonzero(book.nbr_out[:, t] >= 0).flatten()
            book.taps_lists.append((o, book.nbr_out[o, t].long()))
    return book.taps_lists


def torch_forward(f, w, book):
    wt = w.reshape(w.shape[0], -1, w.shape[-1])
    out = f.new_zeros((book.n_out, w.shape[0]))
    for t, (o, i) in enumerate(tap_lists(book)):
        if o.numel():
            out.index_add_(0, o, f.index_select(0, i) @ wt[:, t].t())
    return out


def torch_dgrad(go, w, book):
    wt = w.reshape(w.shape[0], -1, w.shape[-1])
    g = go.new_zeros((book.n_in, w.shape[-1]))
    for t, (o, i) in enumerate(tap_lists(book)):
        if o.numel():
            g.index_add_(0, i, go.index_select(0, o) @ wt[:, t])
    return g


def torch_wgrad(f, go, w, book):
    gw = torch.zeros_like(w).reshape(w.shape[0], -1, w.shape[-1])
    for t, (o, i) in enumerate(tap_lists(book)):
        if o.numel():
            gw[:, t] = go.index_select(0, o).t() @ f.index_select(0, i)
    return gw.reshape(w.shape)


class _TorchConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, w, b, book):
        ctx.save_for_backward(f, w)
        ctx.book, ctx.has_bias = book, b is not None
        out = torch_forward(f, w.detach(), book)
        return out if b is None else out + b

    @staticmethod
    def backward(ctx, go):
        f, w = ctx.saved_tensors
        go = go.contiguous()
        return torch_dgrad(go, w, ctx.book), torch_wgrad(f, go, w, ctx.book), (go.sum(0) if ctx.has_bias else None), None


def timed(variants, warmup, reps):
    """variants: {name: callable}; alternates them call by call.  -> {name: (median ms, min ms)}"""
    times = {k: [] for k in variants}
    for it in range(warmup + reps):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--points', type=int, default=60000)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--only', default=None, choices=[None, 'index', 'forward', 'dgrad', 'wgrad', 'backbone'])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_conv_bench needs the GPU: there is no CPU path to time")
    rng = np.random.default_rng(0)
    pts = scenes(rng, args.batch, args.points)
    packed = torch.from_numpy(np.concatenate(pts)).cuda()
    offs = torch.tensor(np.cumsum([0] + [len(p) for p in pts]), dtype=torch.int64).cuda()
    gen = VoxelGenerator(VS, PCR, 4, 5, 16000)
    voxels, coords, num = collate_voxels(*gen.generate_batch((packed, offs, args.points)))
    grid = grid_size(np.array(PCR, np.float64), np.array(VS)).tolist()
    feats = MeanVFE({}, 4)({'voxels': voxels, 'voxel_num_points': num})['voxel_features']
    shape = [grid[2] + 1, grid[1], grid[0]]
    lines = [dict(stage='input', batch=args.batch, voxels=int(coords.shape[0]), sparse_shape=shape)]
    want = lambda s: args.only in (None, s)

    indices, gen_t = coords.contiguous(), torch.Generator(device='cuda').manual_seed(1)
    for name, kind, cin, cout, k, s, p in LEVELS:
        def build():
            if kind == 'subm':
                return sp.build_subm_rulebook(indices, shape, args.batch, k)
            return sp.build_strided_rulebook(indices, shape, args.batch, k, s, p)
        book = build()
        base = dict(level=name, kind=kind, c_in=cin, c_out=cout, n_in=book.n_in, n_out=book.n_out,
                    pairs=int((book.nbr_out >= 0).sum()))
        if want('index'):
            med, lo = timed({'device': build}, args.warmup, args.reps)['device']
            lines.append(dict(base, stage='index', variant='device', median_ms=med, min_ms=lo))
        f = torch.randn((book.n_in, cin), device='cuda', generator=gen_t)
        w = torch.randn((cout,) + sp._triple(k, 'k') + (cin,), device='cuda', generator=gen_t) * 0.05
        go = torch.randn((book.n_out, cout), device='cuda', generator=gen_t)
        wparam = torch.nn.Parameter(w)
        tap_lists(book)

        def dev_dgrad():
            out = torch.empty((book.n_in, cin), device='cuda')
            subm = book.nbr_in is None
            sp._call("pda_spconv_gemm", go, go.data_ptr(), (book.nbr_out if subm else book.nbr_in).data_ptr(),
                     sp._plane(wparam, True).data_ptr(), None, out.data_ptr(), book.n_in, book.n_out, book.taps, cin, cout, 1,
                     1 if subm else 0)
            return out

        def dev_wgrad():
            gw = torch.empty_like(w)
            ws = sp.workspace("pda_spconv_wgrad_workspace_bytes", (book.n_out, book.taps, cin, cout), "sizes", go.device)
            sp._call("pda_spconv_wgrad", go, f.data_ptr(), go.data_ptr(), book.nbr_out.data_ptr(), book.n_out, book.n_in, book.taps,
                     cin, cout, gw.data_ptr(), None, ws.data_ptr())
            return gw
        stages = {'forward': {'device': lambda: sp.sparse_conv(f, wparam.detach(), None, book), 'torch': lambda: torch_forward(f, w, book)},
                  'dgrad': {'device': dev_dgrad, 'torch': lambda: torch_dgrad(go, w, book)},
                  'wgrad': {'device': dev_wgrad, 'torch': lambda: torch_wgrad(f, go, w, book)}}
        for stage, variants in stages.items():
            if not want(stage):
                continue
            a, b = variants['device'](), variants['torch']()
            diff = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
            for variant, (med, lo) in timed(variants, args.warmup, args.reps).items():
                lines.append(dict(base, stage=stage, variant=variant, median_ms=med, min_ms=lo, device_vs_torch_rel_diff=diff))
        if kind == 'spconv':
            indices, shape = book.out_indices.contiguous(), book.out_shape

    if want('backbone'):
        torch.manual_seed(0)
        model = VoxelBackBone8x(to_attr({}), 4, grid).cuda().train()
        own = sp.sparse_conv

        def step(conv):
            sp.sparse_conv = conv
            try:
                for prm in model.parameters():
                    prm.grad = None
                out = model({'voxel_features': feats, 'voxel_coords': coords, 'batch_size': args.batch})
                (out['encoded_spconv_tensor'].features ** 2).sum().backward()
            finally:
                sp.sparse_conv = own
        torch_conv = lambda f, w, b, book: _TorchConv.apply(f, w, b, book)
        res = timed({'device': lambda: step(own), 'torch': lambda: step(torch_conv)}, args.warmup, max(args.reps // 3, 3))
        for variant, (med, lo) in res.items():
            lines.append(dict(level='VoxelBackBone8x', stage='backbone_fwd_bwd', variant=variant, median_ms=med, min_ms=lo))

    text = "\n".join(json.dumps(line) for line in lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
