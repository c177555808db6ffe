#!/usr/bin/env python
"""Generates tests/golden/stack_pool.npz by running the REFERENCE's own Python composition
(pcdet/ops/pointnet2/pointnet2_stack/pointnet2_utils.py: three_nn_for_vector_pool_by_two_step and
vector_pool_with_voxel_query_op, forward and backward) on the CPU, with its `pointnet2_stack_cuda` extension replaced by a
stub backed by the numpy restatement of the kernels (stack_pool_restatement.py), as make_golden.py does for the batch module.

    python tests/golden/make_stack_pool_golden.py <checkout of the reference>

The reference sources are imported from where they lie; nothing of them is copied.  What is committed is data: small inputs
and the composition's outputs.  Inputs lie on the 1/8 lattice, so every distance and cell index is exact in float32 and the
file does not depend on the contraction mode of the squared distance.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import stack_pool_restatement as ref  # noqa: E402
from reference_loader import as_np as _np, load, np_args, reference_root  # noqa: E402

F32, I32 = np.float32, np.int32


class Stub(types.ModuleType):
    """reference-named entry points on CPU tensors"""
    def __init__(self):
        super().__init__("pointnet2_stack_cuda")
        self.rows = None

    @staticmethod
    def query_stacked_local_neighbor_idxs_wrapper_stack(*args):
        ref.query_stacked_local_neighbor_idxs(*np_args(args))
        return 0

    @staticmethod
    def query_three_nn_by_stacked_local_idxs_wrapper_stack(*args):
        ref.query_three_nn_by_stacked_local_idxs(*np_args(args))
        return 0

    @staticmethod
    def vector_pool_wrapper(*args):
        return ref.vector_pool(*np_args(args))

    def vector_pool_grad_wrapper(self, grad_new_features, point_cnt_of_grid, grouped_idxs, grad_support_features):
        self.rows = _np(grouped_idxs).copy()
        ref.vector_pool_grad(_np(grad_new_features), _np(point_cnt_of_grid), _np(grouped_idxs), _np(grad_support_features))
        return 1


def import_reference(root, stub):
    stack = "ops.pointnet2.pointnet2_stack."
    return load(root, "pcdet", [stack + "pointnet2_utils"], stubs={stack + "pointnet2_stack_cuda": stub}, real_paths=True)[0]


def main():
    stub = Stub()
    pu = import_reference(reference_root(), stub)
    rng = np.random.default_rng(2024)
    xyz_cnt, new_cnt = np.array([170, 130], I32), np.array([70, 50], I32)
    N, M, c_in, ce = int(xyz_cnt.sum()), int(new_cnt.sum()), 8, 4
    d, grid, multiplier = 2.0, (2, 2, 4), 1.5
    G = int(np.prod(grid))
    xyz = (rng.integers(-32, 33, (N, 3)) / 8).astype(F32)
    new_xyz = (rng.integers(-24, 25, (M, 3)) / 8).astype(F32)
    xyz[:6] = new_xyz[:6] + np.array([2, 0, 0], F32)               # on the cube's face and the ball's surface
    xyz[6:12] = new_xyz[:6] + np.array([0, 2, -2], F32)
    new_xyz[-3:] += 24                                             # no neighbours: empty lists, empty cells
    feat = rng.normal(size=(N, c_in)).astype(F32)
    grad_out = rng.normal(size=(M, G * ce)).astype(F32)
    ax = [((np.arange(g) + 0.5) * (2 * d / g) - d) for g in grid]
    centers = (new_xyz[:, None, :] + np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3).astype(F32)[None]).astype(F32)
    out = dict(xyz=xyz, xyz_cnt=xyz_cnt, new_xyz=new_xyz, new_cnt=new_cnt, feat=feat, grad_out=grad_out, centers=centers,
               d=np.float64(d), grid=np.array(grid, I32), ce=np.int32(ce), multiplier=np.float64(multiplier),
               avg_length=np.int32(2), mean_points=np.int32(3))     # both too small: the composition's retry loops run
    t = torch.from_numpy
    cases = []
    for neighbor_type, pooling_type, nsample in [(0, 0, -1), (1, 0, -1), (0, 1, -1), (1, 0, 6)]:
        tag = "n%dp%ds%d" % (neighbor_type, pooling_type, max(nsample, 0))
        cases.append(tag)
        out[tag + "_args"] = np.array([neighbor_type, pooling_type, nsample], I32)
        dist, idx, avg = pu.three_nn_for_vector_pool_by_two_step(t(xyz), t(xyz_cnt), t(new_xyz), t(centers), t(new_cnt), d, nsample,
                                                                 neighbor_type, 2, G, multiplier)
        out[tag + "_nn_dist"], out[tag + "_nn_idx"], out[tag + "_nn_avg"] = dist.numpy(), idx.numpy(), np.int32(int(avg))
        f = t(feat.copy()).requires_grad_(True)
        new_features, new_local_xyz, mean_pts, cnt = pu.vector_pool_with_voxel_query_op(
            t(xyz), t(xyz_cnt), f, t(new_xyz), t(new_cnt), *grid, d, ce, True, 3, nsample, neighbor_type, pooling_type)
        new_features.backward(t(grad_out))
        out[tag + "_out"], out[tag + "_lxyz"] = new_features.detach().numpy(), new_local_xyz.numpy()
        out[tag + "_cnt"], out[tag + "_mean_points"] = cnt.numpy(), np.int32(int(mean_pts[0]))
        out[tag + "_grad"], out[tag + "_rows"] = f.grad.numpy(), stub.rows
        print(tag, "rows", len(stub.rows), "mean points", int(mean_pts[0]), "list length", int(avg),
              "empty lists", int((idx.numpy()[..., 0] == -1).sum()))
    out["cases"] = np.array(cases)
    path = os.path.join(HERE, "stack_pool.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
