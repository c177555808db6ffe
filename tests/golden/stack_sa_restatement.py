"""Plain numpy restatements of the three pointnet2_stack kernels PV-RCNN's modules call and of points_in_boxes_gpu, for
make_pv_rcnn_golden.py's stub of the `pointnet2_stack_cuda` extension and for the float64 restatements of
tests/test_pv_rcnn.py.  Float32 arithmetic in the kernels' operation order; `contract` as in stack_pool_restatement.

The farthest-point sampling breaks ties as the kernels' shared-memory tree does (csrc/fps.hip, fps_tiebreak): thread t of a
block of bs = 2^L threads scans the points t, t + bs, ... with a strict comparison, and every step of the tree keeps the left
operand of two equal distances, so among equal distances the point with the smallest (bit-reversed (k mod bs), k / bs) wins.
The batch kernel runs with bs = opt_n_threads(n), the stacked kernel with bs = 1024 whatever n; where n is a power of two up
to 1024 the two orders are the same."""
import numpy as np

from roi_pool_restatement import MARGIN_GPU, in_box
from stack_pool_restatement import sqdist

F32, I32 = np.float32, np.int32


def starts(cnt):
    cnt = np.asarray(cnt, np.int64)
    return np.cumsum(cnt) - cnt


def ball_query(radius, nsample, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, idx, contract=1):
    """ball_query_gpu.cu (stack): idx (M, nsample) caller-zeroed -> indices LOCAL to the scene in ascending order, short lists
    padded with the first hit, idx[i][0] = -1 for an empty ball."""
    radius2 = F32(radius) * F32(radius)
    ps, qs = starts(xyz_batch_cnt), starts(new_xyz_batch_cnt)
    for b in range(len(xyz_batch_cnt)):
        pts = xyz[ps[b]:ps[b] + int(xyz_batch_cnt[b])]
        for i in range(qs[b], qs[b] + int(new_xyz_batch_cnt[b])):
            hits = np.nonzero(sqdist(pts, new_xyz[i], contract) < radius2)[0][:nsample]
            if len(hits) == 0:
                idx[i, 0] = -1
            else:
                idx[i, :] = hits[0]
                idx[i, :len(hits)] = hits


def opt_n_threads(n):
    """sampling_gpu.cu opt_n_threads: the largest power of two not above n, within [1, 1024]"""
    return max(min(1 << int(np.floor(np.log2(max(n, 1)))), 1024), 1)


def _bitrev(k, bits):
    out = 0
    for i in range(bits):
        out |= ((k >> i) & 1) << (bits - 1 - i)
    return out


def fps(xyz, npoint, block=None, contract=1):
    """farthest_point_sampling_kernel for one scene: from point 0, every round keeps min(temp, d) and takes the farthest point;
    ties as the module docstring says, `block` = the kernel's block size (default: the batch kernel's opt_n_threads(n)).
    npoint > len(xyz) returns the first len(xyz) samples followed by -1 (VoxelSetAbstraction overwrites those rounds with
    repeats)."""
    n = len(xyz)
    block = opt_n_threads(n) if block is None else block
    bits = int(np.log2(block))
    order = np.array([(_bitrev(k % block, bits), k // block) for k in range(n)], np.int64)
    rank = np.lexsort((order[:, 1], order[:, 0])).argsort()              # smaller = preferred
    out = np.full(npoint, -1, I32)
    temp = np.full(n, 1e10, F32)
    old = 0
    out[0] = 0
    for j in range(1, min(npoint, n)):
        temp = np.minimum(temp, sqdist(xyz, xyz[old], contract))
        winners = np.nonzero(temp == temp.max())[0]
        old = int(winners[np.argmin(rank[winners])])
        out[j] = old
    return out


def points_in_boxes_gpu(points, boxes, contract=1):
    """roiaware_pool3d_kernel.cu points_in_boxes_kernel: points (B, M, 3), boxes (B, T, 7) -> (B, M) int32, the index of the
    first box that holds the point, -1 for none."""
    B, M = points.shape[:2]
    out = np.full((B, M), -1, I32)
    for b in range(B):
        for t in range(boxes.shape[1] - 1, -1, -1):
            hit, _, _ = in_box(points[b], boxes[b, t], MARGIN_GPU, contract)
            out[b, hit] = t
    return out
