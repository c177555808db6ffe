#!/usr/bin/env python
"""Times the voxel-query and vector-pool entries of the pointnet2_stack operator set (csrc/stack_pool.hip), one device-event
pair around every launch, median and minimum of --iters launches after --warmup launches.

PV-RCNN++-like shape: 2 scenes of 16 384 support points and 4 096 centres each (centres are support points), uniform in a
70 m x 80 m x 4 m slab, C_in = 32, grid 3 x 3 x 3, d = 2.4, both neighbourhood types; num_c_out_each_grid 32 (no fold) and
2 (sixteen-fold): query_stacked_local_neighbor_idxs (d * 1.5, three launches), query_three_nn_by_stacked_local_idxs,
vector_pool (both pooling types; outputs re-zeroed outside the timed span), vector_pool_grad.
Voxel-RCNN-like voxel_query: 2 scenes, grid 41 x 1600 x 1408 (voxels 0.05 x 0.05 x 0.1), 120 000 occupied voxels a scene,
occupied voxels in a band of four z layers, 55 296 centres (128 boxes x 216 grid points a scene) next to them, range (4, 4, 4), radius 0.4, nsample 16.
Prints one JSON line per entry and variant.  Needs a GPU.

    python tools/stack_pool_bench.py [--iters 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdanet_amd import pointnet2_stack_cuda as ext  # noqa: E402
from pdanet_amd.pointnet2_batch_cuda import _call  # noqa: E402


def timed(fn, reset, iters, warmup):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for i in range(warmup + iters):
        reset()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "launches": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "stack_pool_bench needs a GPU"
    dev = torch.device("cuda")
    name = torch.cuda.get_device_name(0)
    rng = np.random.default_rng(0)
    i32 = dict(dtype=torch.int32, device=dev)

    def emit(**line):
        line["device"] = name
        print(json.dumps(line), flush=True)

    # ---- PV-RCNN++-like vector pool ----------------------------------------------------------------------------------
    B, n_per, m_per, c_in, grid, d = 2, 16384, 4096, 32, (3, 3, 3), 2.4
    G = int(np.prod(grid))
    pts = np.stack([rng.uniform(0, 70, B * n_per), rng.uniform(-40, 40, B * n_per), rng.uniform(-3, 1, B * n_per)], 1).astype(np.float32)
    ctr = np.concatenate([pts[b * n_per: b * n_per + m_per] for b in range(B)])
    xyz, new_xyz = torch.from_numpy(pts).to(dev), torch.from_numpy(ctr).to(dev)
    feat = torch.from_numpy(rng.normal(size=(B * n_per, c_in)).astype(np.float32)).to(dev)
    cnt, ncnt = torch.full((B,), n_per, **i32), torch.full((B,), m_per, **i32)
    N, M = B * n_per, B * m_per
    ax = [((np.arange(g) + 0.5) * (2 * d / g) - d) for g in grid]
    off = torch.from_numpy(np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)).to(dev)
    centers = (new_xyz[:, None, :] + off[None]).contiguous()
    shape = {"scenes": B, "support_per_scene": n_per, "centres_per_scene": m_per, "c_in": c_in, "grid": list(grid), "d": d}
    for neighbor_type in (0, 1):
        kind = "ball" if neighbor_type == 1 else "cube"
        # neighbour lists at d * 1.5, then the three nearest of every grid point
        avg = 1000
        lst, sl, cs = torch.zeros(avg * M, **i32), torch.zeros((M, 2), **i32), torch.zeros(1, **i32)
        t = timed(lambda: ext.query_stacked_local_neighbor_idxs_wrapper_stack(xyz, cnt, new_xyz, ncnt, lst, sl, cs, avg, d * 1.5, -1,
                                                                              neighbor_type), cs.zero_, a.iters, a.warmup)
        total = int(cs[0])
        emit(entry="query_stacked_local_neighbor_idxs", neighbourhood=kind, **shape, list_entries=total,
             longest_list=int(sl[:, 1].max()), **t)
        idx, d2 = torch.full((M, G, 3), -1, **i32), torch.zeros((M, G, 3), device=dev)
        lst_fit = lst[:total].contiguous()
        t = timed(lambda: ext.query_three_nn_by_stacked_local_idxs_wrapper_stack(xyz, new_xyz, centers, idx, d2, lst_fit, sl, M, G),
                  lambda: None, a.iters, a.warmup)
        emit(entry="query_three_nn_by_stacked_local_idxs", neighbourhood=kind, **shape, list_entries=total, **t)
        for ce in (32, 2):
            for pooling_type in (0, 1):
                rows = 200 * M
                nf, nl = torch.zeros((M, G * ce), device=dev), torch.zeros((M, 3 * G), device=dev)
                pc, gi, word = torch.zeros((M, G), **i32), torch.zeros((rows, 3), **i32), torch.zeros(1, **i32)

                def reset():
                    nf.zero_(); nl.zero_(); pc.zero_()

                def pool():
                    _call("pda_stack_vector_pool", xyz, xyz.data_ptr(), feat.data_ptr(), cnt.data_ptr(), new_xyz.data_ptr(),
                          ncnt.data_ptr(), nf.data_ptr(), nl.data_ptr(), pc.data_ptr(), gi.data_ptr(), word.data_ptr(), B, M, c_in,
                          G * ce, G, *grid, d, 1, rows, -1, neighbor_type, pooling_type)
                t = timed(pool, reset, a.iters, a.warmup)
                total_rows = int(word[0])
                assert total_rows <= rows
                emit(entry="vector_pool", neighbourhood=kind, pooling_type=pooling_type, num_c_out_each_grid=ce, **shape,
                     rows=total_rows, **t)
                if pooling_type == 0:
                    g_out = torch.from_numpy(rng.normal(size=(M, G * ce)).astype(np.float32)).to(dev)
                    g_in = torch.zeros((N, c_in), device=dev)
                    gi_fit = gi[:total_rows].contiguous()
                    t = timed(lambda: ext.vector_pool_grad_wrapper(g_out, pc, gi_fit, g_in), g_in.zero_, a.iters, a.warmup)
                    emit(entry="vector_pool_grad", neighbourhood=kind, num_c_out_each_grid=ce, **shape, rows=total_rows, **t)
                del nf, nl, pc, gi
    del lst, feat, centers

    # ---- Voxel-RCNN-like voxel query ---------------------------------------------------------------------------------
    R, vs, lo = (41, 1600, 1408), np.array([0.05, 0.05, 0.1]), np.array([0.0, -40.0, -3.0])
    n_vox, m_q = 120000, 128 * 216
    pi = torch.full((B,) + R, -1, **i32)
    vox_xyz, q_xyz, q_coords = [], [], []
    for b in range(B):
        c = np.unique(np.stack([rng.integers(0, R[2], 2 * n_vox), rng.integers(0, R[1], 2 * n_vox), rng.integers(10, 14, 2 * n_vox)], 1), axis=0)
        c = c[rng.permutation(len(c))[:n_vox]]                                  # x, y, z voxel coordinates of occupied voxels
        base = b * n_vox
        pi[b, torch.from_numpy(c[:, 2]).to(dev), torch.from_numpy(c[:, 1]).to(dev), torch.from_numpy(c[:, 0]).to(dev)] = \
            torch.arange(base, base + len(c), **i32)
        p = (c + 0.5) * vs + lo
        vox_xyz.append(p)
        q = p[rng.integers(0, len(p), m_q)] + rng.uniform(-0.2, 0.2, (m_q, 3))
        qc = np.clip(np.floor((q - lo) / vs).astype(np.int64), 0, [R[2] - 1, R[1] - 1, R[0] - 1])
        q_xyz.append(q)
        q_coords.append(np.stack([np.full(m_q, b), qc[:, 2], qc[:, 1], qc[:, 0]], 1))
    vxyz = torch.from_numpy(np.concatenate(vox_xyz).astype(np.float32)).to(dev)
    qxyz = torch.from_numpy(np.concatenate(q_xyz).astype(np.float32)).to(dev)
    qcoords = torch.from_numpy(np.concatenate(q_coords).astype(np.int32)).to(dev)
    Mq, ns = qxyz.shape[0], 16
    idx = torch.zeros((Mq, ns), **i32)
    t = timed(lambda: ext.voxel_query_wrapper(Mq, *R, ns, 0.4, 4, 4, 4, qxyz, vxyz, qcoords, pi, idx), idx.zero_, a.iters, a.warmup)
    emit(entry="voxel_query", scenes=B, grid=list(R), occupied_voxels_per_scene=n_vox, centres=Mq, range=[4, 4, 4], radius=0.4,
         nsample=ns, empty_balls=int((idx[:, 0] == -1).sum()), full_rows=int((idx[:, -1] != idx[:, 0]).sum()), **t)


if __name__ == "__main__":
    main()
