"""Plain numpy restatement of the reference's roiaware_pool3d_kernel.cu:16-310, roipoint_pool3d_kernel.cu:15-165 and the
host test of roiaware_pool3d.cpp:121-168: float32 arithmetic with explicit intermediate casts, sequential, one function per
entry point of the extension modules, the reference's argument order and allocation contracts (outputs are written in place
into caller-allocated, zero-filled arrays).

The box test is the one of csrc/box_rec.h: cos(-rz) and sin(-rz) are taken in double and rounded to float, the limits
dx / 2.0 + MARGIN are double expressions, and `contract` selects the float expression of the local coordinates:
1 = fma(sx, cosa, sy * -sina), 0 = sx * cosa + sy * -sina.  The reference leaves the order of the float atomics of the
backward open; roiaware_pool3d_backward_terms returns, per element of grad_in, the float64 sum of the terms, the sum of
their magnitudes and their number, and roiaware_pool3d_backward stores the float64 sum rounded once."""
import numpy as np

F32, I32, F64 = np.float32, np.int32, np.float64
MARGIN_GPU = F64(F32(1e-5))                        # check_pt_in_box3d on the device
MARGIN_CPU = F64(F32(1e-2))                        # check_pt_in_box3d_cpu on the host


def _fma(a, b, c):
    # float32 fma through float64: a * b is exact there; the sum is rounded to 53 bits, then to 24
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


def in_box(pts, box, margin, contract):
    """pts (P, 3) float32, box (7) float32 -> (hit (P) bool, local_x (P) float32, local_y (P) float32)"""
    pts, box = np.asarray(pts, F32), np.asarray(box, F32)
    cx, cy, cz, dx, dy, dz, rz = box
    cosa, sina = F32(np.cos(F64(-rz))), F32(np.sin(F64(-rz)))
    z_in = ~(np.abs((pts[:, 2] - cz).astype(F32)) > F32(dz * F32(0.5)))
    sx, sy = (pts[:, 0] - cx).astype(F32), (pts[:, 1] - cy).astype(F32)
    if contract:
        lx = _fma(sx, cosa, (sy * F32(-sina)).astype(F32))
        ly = _fma(sx, sina, (sy * cosa).astype(F32))
    else:
        lx = ((sx * cosa).astype(F32) + (sy * F32(-sina)).astype(F32)).astype(F32)
        ly = ((sx * sina).astype(F32) + (sy * cosa).astype(F32)).astype(F32)
    hit = z_in & (np.abs(lx).astype(F64) < F64(dx) / 2.0 + margin) & (np.abs(ly).astype(F64) < F64(dy) / 2.0 + margin)
    return hit, lx, ly


def voxel_axis(local, d, out):
    """roiaware_pool3d_kernel.cu:60-70 for one axis: float32 division, float32 sum, float32 division, truncation, and the
    clamp on an UNSIGNED value: a negative index wraps and lands in the last voxel"""
    res = F32(F32(d) / F32(out))
    val = F32(F32(F32(local) + F32(F32(d) / F32(2))) / res)
    return min(int(val) & 0xFFFFFFFF, out - 1)


def roiaware_pool3d_forward(rois, pts, pts_feature, argmax, pts_idx_of_voxels, pooled_features, pool_method, contract=1):
    n_box, out_x, out_y, out_z, k_slots = pts_idx_of_voxels.shape
    for b in range(n_box):
        hit, lx, ly = in_box(pts, rois[b], MARGIN_GPU, contract)
        dx, dy, dz = rois[b, 3], rois[b, 4], rois[b, 5]
        for k in np.nonzero(hit)[0]:                                   # ascending point index
            xi, yi = voxel_axis(lx[k], dx, out_x), voxel_axis(ly[k], dy, out_y)
            zi = voxel_axis(F32(pts[k, 2] - rois[b, 2]), dz, out_z)
            slots = pts_idx_of_voxels[b, xi, yi, zi]
            cnt = int(slots[0])
            if cnt < k_slots - 1:
                slots[cnt + 1] = k
                slots[0] = cnt + 1
        if pool_method == 0:
            argmax[b] = -1                                             # written for every voxel, empty ones included
        for xi, yi, zi in zip(*np.nonzero(pts_idx_of_voxels[b, ..., 0])):
            slots = pts_idx_of_voxels[b, xi, yi, zi]
            if pool_method == 0:
                best = np.full(pts_feature.shape[1], -np.inf, F32)     # the reference's -1e50 is -inf in float
                arg = np.full(pts_feature.shape[1], -1, I32)
                for s in range(1, int(slots[0]) + 1):
                    f = pts_feature[slots[s]]
                    take = f > best                                    # strict: ties keep the lower slot; NaN, -inf never win
                    best, arg = np.where(take, f, best), np.where(take, slots[s], arg).astype(I32)
                keep = arg != -1
                pooled_features[b, xi, yi, zi][keep] = best[keep]
                argmax[b, xi, yi, zi] = arg
            else:
                total = np.zeros(pts_feature.shape[1], F32)
                for s in range(1, int(slots[0]) + 1):
                    total = (total + pts_feature[slots[s]]).astype(F32)
                pooled_features[b, xi, yi, zi] = (total / F32(int(slots[0]))).astype(F32)
    return 1


def roiaware_pool3d_backward_terms(pts_idx_of_voxels, argmax, grad_out, num_pts, pool_method):
    """-> (float64 sum of the terms, sum of their magnitudes, number of terms), each (num_pts, C).  A term is grad_out at an
    argmax (max) or grad_out / count for every slot of a voxel (avg), in exact arithmetic up to float64."""
    c = grad_out.shape[-1]
    s, a, n = np.zeros((num_pts, c), F64), np.zeros((num_pts, c), F64), np.zeros((num_pts, c), np.int64)
    ch = np.arange(c)
    go = grad_out.reshape(-1, c).astype(F64)
    if pool_method == 0:
        am = argmax.reshape(-1, c)
        for v in np.nonzero((am != -1).any(axis=1))[0]:
            ok = am[v] != -1
            np.add.at(s, (am[v][ok], ch[ok]), go[v][ok])
            np.add.at(a, (am[v][ok], ch[ok]), np.abs(go[v][ok]))
            np.add.at(n, (am[v][ok], ch[ok]), 1)
    else:
        slots = pts_idx_of_voxels.reshape(-1, pts_idx_of_voxels.shape[-1])
        for v in np.nonzero(slots[:, 0])[0]:
            cnt = int(slots[v, 0])
            for p in slots[v, 1:cnt + 1]:
                s[p] += go[v] / cnt
                a[p] += np.abs(go[v]) / cnt
                n[p] += 1
    return s, a, n


def roiaware_pool3d_backward(pts_idx_of_voxels, argmax, grad_out, grad_in, pool_method):
    s, _, _ = roiaware_pool3d_backward_terms(pts_idx_of_voxels, argmax, grad_out, grad_in.shape[0], pool_method)
    grad_in += s.astype(F32)
    return 1


def points_in_boxes_cpu(boxes, pts, pts_indices):
    """roiaware_pool3d.cpp:143-168: (N, 7), (P, 3) -> pts_indices (N, P) of 0 / 1; margin 1e-2, no FMA (host code)"""
    for i in range(boxes.shape[0]):
        pts_indices[i] = in_box(pts, boxes[i], MARGIN_CPU, 0)[0]
    return 1


def roipoint_pool3d_forward(xyz, boxes3d, pts_feature, pooled_features, pooled_empty_flag, contract=1):
    """xyz (B, P, 3), boxes3d (B, M, 7) already enlarged, pts_feature (B, P, C) -> pooled_features (B, M, S, 3 + C),
    pooled_empty_flag (B, M)"""
    n_sample = pooled_features.shape[2]
    for bs in range(xyz.shape[0]):
        for m in range(boxes3d.shape[1]):
            picked = np.nonzero(in_box(xyz[bs], boxes3d[bs, m], MARGIN_GPU, contract)[0])[0][:n_sample]
            cnt = len(picked)
            if cnt == 0:
                pooled_empty_flag[bs, m] = 1                           # the rows stay as they were
                continue
            for k in range(n_sample):
                p = picked[k] if k < cnt else picked[k % cnt]          # duplicate the same points for sampling
                pooled_features[bs, m, k, :3] = xyz[bs, p]
                pooled_features[bs, m, k, 3:] = pts_feature[bs, p]
    return 1
