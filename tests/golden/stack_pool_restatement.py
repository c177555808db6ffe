"""Plain numpy restatement of the reference's voxel_query_gpu.cu:10-89 and vector_pool_gpu.cu:19-458: float32 arithmetic
in the kernels' operation order, one function per kernel, the reference's argument order and allocation contracts (outputs
are written in place into caller-allocated arrays).  `contract` selects the float expression of the squared distance:
1 = fma(dz, dz, fma(dy, dy, dx * dx)), 0 = (dx * dx + dy * dy) + dz * dz (csrc/pda_common.h sqdist3).

Where the reference leaves something to the order in which threads run, this file fixes it the way the library does:
starts of the neighbour lists follow the centre order, and rows of grouped_idxs are compared as a set.  vector_pool_grad is
evaluated in float64 (the kernel's float atomics have no defined order)."""
import numpy as np

F32, I32 = np.float32, np.int32
MAX_CANDIDATES = 1000


def _fma(a, b, c):
    # float32 fma through float64: a * b is exact there; the sum is rounded to 53 bits, then to 24
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def sqdist(a, b, contract):
    """squared distance of float32 points a - b (..., 3), the kernels' expression"""
    d = (np.asarray(a, F32) - np.asarray(b, F32)).astype(F32)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    if contract:
        return _fma(dz, dz, _fma(dy, dy, (dx * dx).astype(F32)))
    return ((dx * dx + dy * dy).astype(F32) + dz * dz).astype(F32)


def _scene_of(cnt, i):
    # vector_pool_gpu.cu:140-145: indices past the total stay in the last scene
    bs, pt_cnt = 0, int(cnt[0])
    for k in range(1, len(cnt)):
        if i < pt_cnt:
            break
        pt_cnt += int(cnt[k])
        bs = k
    return bs


def _hits(support, q, d, neighbor_type, contract):
    """ascending local indices of the scene's points that pass the ball (1) or cube test, and their local coordinates"""
    local = (support - q).astype(F32)
    if neighbor_type == 1:
        skip = sqdist(support, q, contract) > F32(d) * F32(d)
    else:
        skip = (np.abs(local) > F32(d)).any(axis=1)
    ks = np.nonzero(~skip)[0]
    return ks, local[ks]


def voxel_query(M, R1, R2, R3, nsample, radius, z_range, y_range, x_range, new_xyz, xyz, new_coords, point_indices, idx,
                contract=1):
    radius2 = F32(radius) * F32(radius)
    pi = point_indices.reshape(-1, R1, R2, R3)
    for m in range(M):
        b, cz, cy, cx = (int(v) for v in new_coords[m])
        zs = [z for z in range(cz - z_range, cz + z_range + 1) if 0 <= z < R1]
        ys = [y for y in range(cy - y_range, cy + y_range + 1) if 0 <= y < R2]
        xs = [x for x in range(cx - x_range, cx + x_range + 1) if 0 <= x < R3]
        cnt = 0
        if zs and ys and xs:
            cells = pi[b][np.ix_(zs, ys, xs)].ravel()              # dz, dy, dx in that nesting
            cand = cells[cells >= 0]
            cand = cand[~(sqdist(xyz[cand], new_xyz[m], contract) > radius2)]
            for g in cand:
                if cnt < nsample:
                    if cnt == 0:
                        idx[m, :] = g
                    idx[m, cnt] = g
                    cnt += 1
        if cnt == 0:
            idx[m, 0] = -1


def query_stacked_local_neighbor_idxs(support_xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, stack_neighbor_idxs, start_len,
                                      cumsum, avg_length_of_neighbor_idxs, max_neighbour_distance, nsample, neighbor_type,
                                      contract=1):
    M = new_xyz.shape[0]
    starts = np.concatenate([[0], np.cumsum(xyz_batch_cnt)]).astype(np.int64)
    max_thresh = avg_length_of_neighbor_idxs * M
    for m in range(M):
        bs = _scene_of(new_xyz_batch_cnt, m)
        s0, n = int(starts[bs]), int(xyz_batch_cnt[bs])
        ks, _ = _hits(support_xyz[s0:s0 + n], new_xyz[m], max_neighbour_distance, neighbor_type, contract)
        ks = ks[:MAX_CANDIDATES]                                   # the 1001st candidate breaks with the count at 1000
        if nsample > 0:
            ks = ks[:nsample]
        start = int(cumsum[0])                                     # centre order instead of the atomic counter
        cumsum[0] += len(ks)
        start_len[m] = (start, len(ks))
        if start >= max_thresh:
            continue
        ks = ks[:max(min(len(ks), max_thresh - start), 0)]
        stack_neighbor_idxs[start:start + len(ks)] = ks + s0


def query_three_nn_by_stacked_local_idxs(support_xyz, new_xyz, new_xyz_grid_centers, new_xyz_grid_idxs, new_xyz_grid_dist2,
                                         stack_neighbor_idxs, start_len, M, num_total_grids, contract=1):
    centers = new_xyz_grid_centers.reshape(M, num_total_grids, 3)
    start, length = start_len[:, 0].astype(np.int64), start_len[:, 1].astype(np.int64)
    best = np.full((3, M, num_total_grids), 1e40, np.float64)      # best* are double in the reference
    besti = np.full((3, M, num_total_grids), -1, np.int64)
    for k in range(int(length.max()) if M else 0):                 # list order, every (centre, grid) pair at once
        on = (k < length)
        cur = np.where(on, stack_neighbor_idxs[np.where(on, start + k, 0)] if len(stack_neighbor_idxs) else 0, 0)
        d = sqdist(centers, support_xyz[cur][:, None, :], contract).astype(np.float64)
        on = np.broadcast_to(on[:, None], d.shape)
        curg = np.broadcast_to(cur[:, None], d.shape)
        c1 = on & (d < best[0])
        c2 = on & ~c1 & (d < best[1])
        c3 = on & ~c1 & ~c2 & (d < best[2])
        shift = c1 | c2
        best[2], besti[2] = np.where(shift, best[1], np.where(c3, d, best[2])), np.where(shift, besti[1], np.where(c3, curg, besti[2]))
        best[1], besti[1] = np.where(c1, best[0], np.where(c2, d, best[1])), np.where(c1, besti[0], np.where(c2, curg, besti[1]))
        best[0], besti[0] = np.where(c1, d, best[0]), np.where(c1, curg, besti[0])
    for j in (1, 2):                                               # a missing second or third neighbour repeats the first
        miss = besti[j] == -1
        besti[j], best[j] = np.where(miss, besti[0], besti[j]), np.where(miss, best[0], best[j])
    with np.errstate(over="ignore"):
        new_xyz_grid_dist2.reshape(M, num_total_grids, 3)[...] = np.moveaxis(best, 0, -1).astype(F32)   # float(1e40) = inf
    new_xyz_grid_idxs.reshape(M, num_total_grids, 3)[...] = np.moveaxis(besti, 0, -1)


def vector_pool(support_xyz, xyz_batch_cnt, support_features, new_xyz, new_xyz_batch_cnt, new_features, new_local_xyz,
                point_cnt_of_grid, grouped_idxs, num_grid_x, num_grid_y, num_grid_z, max_neighbour_distance, use_xyz,
                num_max_sum_points, nsample, neighbor_type, pooling_type, contract=1):
    M, num_c_in = new_xyz.shape[0], support_features.shape[1]
    num_c_out, num_total_grids = new_features.shape[1], point_cnt_of_grid.shape[1]
    ce = num_c_out // num_total_grids
    d = F32(max_neighbour_distance)
    gs = np.array([d * F32(2) / F32(num_grid_x), d * F32(2) / F32(num_grid_y), d * F32(2) / F32(num_grid_z)], F32)
    starts = np.concatenate([[0], np.cumsum(xyz_batch_cnt)]).astype(np.int64)
    feats = new_features.reshape(M, num_total_grids, ce)
    lxyz = new_local_xyz.reshape(M, num_total_grids, 3)
    cum_sum = 0
    for m in range(M):
        bs = _scene_of(new_xyz_batch_cnt, m)
        s0, n = int(starts[bs]), int(xyz_batch_cnt[bs])
        ks, local = _hits(support_xyz[s0:s0 + n], new_xyz[m], max_neighbour_distance, neighbor_type, contract)
        g = np.floor(((local + d).astype(F32) / gs).astype(F32)).astype(np.int64)        # true float divisions
        cells = g[:, 0] * num_grid_y * num_grid_z + g[:, 1] * num_grid_z + g[:, 2]
        cells = np.minimum(np.maximum(cells, 0), num_total_grids - 1)                      # clamp on the linear index only
        sample_cnt = 0
        for k, loc, cell in zip(ks, local, cells):
            if pooling_type == 0:
                point_cnt_of_grid[m, cell] += 1
                for i0 in range(0, num_c_in, ce):                  # i ascending: channels fold onto the cell's ce outputs
                    w = min(ce, num_c_in - i0)
                    feats[m, cell, :w] += support_features[s0 + k, i0:i0 + w]
                if use_xyz:
                    lxyz[m, cell] += loc
            elif pooling_type == 1:
                if point_cnt_of_grid[m, cell] != 0:
                    continue
                point_cnt_of_grid[m, cell] += 1
                for i0 in range(0, num_c_in, ce):
                    w = min(ce, num_c_in - i0)
                    feats[m, cell, :w] = support_features[s0 + k, i0:i0 + w]
                if use_xyz:
                    lxyz[m, cell] = loc
            else:
                continue
            cnt = cum_sum
            cum_sum += 1
            if cnt >= num_max_sum_points:
                continue                                           # keeps counting
            grouped_idxs[cnt] = (s0 + k, m, cell)
            sample_cnt += 1
            if nsample > 0 and sample_cnt >= nsample:
                break
            if pooling_type == 1 and sample_cnt >= num_total_grids:
                break
    return cum_sum


def vector_pool_grad(grad_new_features, point_cnt_of_grid, grouped_idxs, grad_support_features):
    """float64 evaluation; returns (per-element number of terms, per-element sum of |terms|) for the caller's error bound"""
    num_c_in = grad_support_features.shape[1]
    M, num_c_out = grad_new_features.shape
    num_total_grids = point_cnt_of_grid.shape[1]
    ce = num_c_out // num_total_grids
    g = grad_new_features.reshape(M, num_total_grids, ce)
    k, m, cell = (grouped_idxs[:, j].astype(np.int64) for j in range(3))
    cnt = np.maximum(point_cnt_of_grid[m, cell].astype(F32), F32(1.0))
    fold = np.arange(num_c_in) % ce
    terms = g[m, cell][:, fold].astype(np.float64) / cnt[:, None].astype(np.float64)
    acc = np.zeros(grad_support_features.shape, np.float64)
    n_terms = np.zeros(grad_support_features.shape, np.int64)
    mag = np.zeros(grad_support_features.shape, np.float64)
    np.add.at(acc, k, terms)
    np.add.at(n_terms, k, 1)
    np.add.at(mag, k, np.abs(terms))
    grad_support_features += acc.astype(grad_support_features.dtype)
    return n_terms, mag
