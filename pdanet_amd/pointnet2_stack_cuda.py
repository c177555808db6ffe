"""Drop-in for the reference's `pointnet2_stack_cuda` extension
(pcdet/ops/pointnet2/pointnet2_stack/src/pointnet2_api.cpp:12-31): same entry-point names, positional
arguments and return conventions, on libpda_pointnet2.so (include/pda_pointnet2_stack.h)."""
import torch

from . import pointnet2_batch_cuda as _batch
from .pointnet2_batch_cuda import F32, I32, _call, _chk, _numel_ok


def ball_query_wrapper(B, M, radius, nsample, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, idx):
    _numel_ok(new_xyz, M * 3, "new_xyz"); _numel_ok(idx, M * nsample, "idx")
    _numel_ok(new_xyz_batch_cnt, B, "new_xyz_batch_cnt"); _numel_ok(xyz_batch_cnt, B, "xyz_batch_cnt")
    _call("pda_stack_ball_query", xyz, _chk(new_xyz, "new_xyz", F32), _chk(new_xyz_batch_cnt, "new_xyz_batch_cnt", I32),
          _chk(xyz, "xyz", F32), _chk(xyz_batch_cnt, "xyz_batch_cnt", I32), _chk(idx, "idx", I32), B, M, float(radius), nsample)
    return 1


def group_points_wrapper(B, M, C, nsample, features, features_batch_cnt, idx, idx_batch_cnt, out):
    _numel_ok(idx, M * nsample, "idx"); _numel_ok(out, M * C * nsample, "out")
    _numel_ok(features_batch_cnt, B, "features_batch_cnt"); _numel_ok(idx_batch_cnt, B, "idx_batch_cnt")
    _call("pda_stack_group_points", features, _chk(features, "features", F32), _chk(features_batch_cnt, "features_batch_cnt", I32),
          _chk(idx, "idx", I32), _chk(idx_batch_cnt, "idx_batch_cnt", I32), _chk(out, "out", F32), B, M, C, nsample)
    return 1


def group_points_grad_wrapper(B, M, C, N, nsample, grad_out, idx, idx_batch_cnt, features_batch_cnt, grad_features):
    _numel_ok(grad_out, M * C * nsample, "grad_out"); _numel_ok(idx, M * nsample, "idx"); _numel_ok(grad_features, N * C, "grad_features")
    _call("pda_stack_group_points_grad", grad_out, _chk(grad_out, "grad_out", F32), _chk(idx, "idx", I32),
          _chk(idx_batch_cnt, "idx_batch_cnt", I32), _chk(features_batch_cnt, "features_batch_cnt", I32),
          _chk(grad_features, "grad_features", F32), B, M, C, N, nsample)
    return 1


farthest_point_sampling_wrapper = _batch.farthest_point_sampling_wrapper      # (B, N, 3) batch layout (:16)


def stack_farthest_point_sampling_wrapper(xyz, temp, xyz_batch_cnt, idx, num_sampled_points):
    B = xyz_batch_cnt.shape[0]
    _numel_ok(temp, xyz.shape[0], "temp"); _numel_ok(num_sampled_points, B, "num_sampled_points")
    _call("pda_stack_furthest_point_sampling", xyz, _chk(xyz, "xyz", F32), _chk(temp, "temp", F32),
          _chk(xyz_batch_cnt, "xyz_batch_cnt", I32), _chk(idx, "idx", I32), _chk(num_sampled_points, "num_sampled_points", I32), B)
    return 1


def three_nn_wrapper(unknown, unknown_batch_cnt, known, known_batch_cnt, dist2, idx):
    B, N = unknown_batch_cnt.shape[0], unknown.shape[0]
    _numel_ok(dist2, N * 3, "dist2"); _numel_ok(idx, N * 3, "idx"); _numel_ok(known_batch_cnt, B, "known_batch_cnt")
    _call("pda_stack_three_nn", unknown, _chk(unknown, "unknown", F32), _chk(unknown_batch_cnt, "unknown_batch_cnt", I32),
          _chk(known, "known", F32), _chk(known_batch_cnt, "known_batch_cnt", I32), _chk(dist2, "dist2", F32),
          _chk(idx, "idx", I32), B, N)


def three_interpolate_wrapper(features, idx, weight, out):
    N, C = idx.shape[0], features.shape[1]
    _numel_ok(weight, N * 3, "weight"); _numel_ok(out, N * C, "out")
    _call("pda_stack_three_interpolate", features, _chk(features, "features", F32), _chk(idx, "idx", I32),
          _chk(weight, "weight", F32), _chk(out, "out", F32), N, C)


def three_interpolate_grad_wrapper(grad_out, idx, weight, grad_features):
    N, C = grad_out.shape[0], grad_out.shape[1]
    _numel_ok(idx, N * 3, "idx"); _numel_ok(weight, N * 3, "weight")
    _call("pda_stack_three_interpolate_grad", grad_out, _chk(grad_out, "grad_out", F32), _chk(idx, "idx", I32),
          _chk(weight, "weight", F32), _chk(grad_features, "grad_features", F32), N, C)


def voxel_query_wrapper(M, R1, R2, R3, nsample, radius, z_range, y_range, x_range, new_xyz, xyz, new_coords, point_indices, idx):
    """voxel_query.cpp:28: idx (M, nsample) zero-filled by the caller -> GLOBAL rows of xyz, idx[:, 0] = -1 for an empty ball."""
    _numel_ok(new_xyz, M * 3, "new_xyz"); _numel_ok(new_coords, M * 4, "new_coords"); _numel_ok(idx, M * nsample, "idx")
    cells = R1 * R2 * R3
    B = point_indices.numel() // cells if cells > 0 else 0
    _call("pda_stack_voxel_query", xyz, _chk(new_xyz, "new_xyz", F32), _chk(xyz, "xyz", F32), _chk(new_coords, "new_coords", I32),
          _chk(point_indices, "point_indices", I32), _chk(idx, "idx", I32), B, xyz.shape[0], M, R1, R2, R3, nsample,
          float(radius), z_range, y_range, x_range)
    return 1


def query_stacked_local_neighbor_idxs_wrapper_stack(support_xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, stack_neighbor_idxs,
                                                    start_len, cumsum, avg_length_of_neighbor_idxs, max_neighbour_distance,
                                                    nsample, neighbor_type):
    """vector_pool.cpp:35: start_len (M, 2) = [start, count], lists at stack_neighbor_idxs[start ...], cumsum[0] += total."""
    B, M = xyz_batch_cnt.shape[0], new_xyz.shape[0]
    _numel_ok(new_xyz_batch_cnt, B, "new_xyz_batch_cnt"); _numel_ok(start_len, M * 2, "start_len"); _numel_ok(cumsum, 1, "cumsum")
    _numel_ok(stack_neighbor_idxs, avg_length_of_neighbor_idxs * M, "stack_neighbor_idxs")
    _call("pda_stack_query_local_neighbor_idxs", support_xyz, _chk(support_xyz, "support_xyz", F32),
          _chk(xyz_batch_cnt, "xyz_batch_cnt", I32), _chk(new_xyz, "new_xyz", F32), _chk(new_xyz_batch_cnt, "new_xyz_batch_cnt", I32),
          _chk(stack_neighbor_idxs, "stack_neighbor_idxs", I32), _chk(start_len, "start_len", I32), _chk(cumsum, "cumsum", I32),
          avg_length_of_neighbor_idxs, float(max_neighbour_distance), B, M, nsample, neighbor_type)
    return 0


def query_three_nn_by_stacked_local_idxs_wrapper_stack(support_xyz, new_xyz, new_xyz_grid_centers, new_xyz_grid_idxs,
                                                       new_xyz_grid_dist2, stack_neighbor_idxs, start_len, M, num_total_grids):
    """vector_pool.cpp:78: (M, num_total_grids, 3) indices and squared distances of the three nearest list entries."""
    _numel_ok(new_xyz, M * 3, "new_xyz"); _numel_ok(start_len, M * 2, "start_len")
    for t, name in ((new_xyz_grid_centers, "new_xyz_grid_centers"), (new_xyz_grid_idxs, "new_xyz_grid_idxs"),
                    (new_xyz_grid_dist2, "new_xyz_grid_dist2")):
        _numel_ok(t, M * num_total_grids * 3, name)
    _call("pda_stack_three_nn_by_local_idxs", support_xyz, _chk(support_xyz, "support_xyz", F32),
          _chk(new_xyz_grid_centers, "new_xyz_grid_centers", F32), _chk(new_xyz_grid_idxs, "new_xyz_grid_idxs", I32),
          _chk(new_xyz_grid_dist2, "new_xyz_grid_dist2", F32), _chk(stack_neighbor_idxs, "stack_neighbor_idxs", I32),
          _chk(start_len, "start_len", I32), support_xyz.shape[0], stack_neighbor_idxs.numel(), M, num_total_grids)
    return 0


def vector_pool_wrapper(support_xyz, xyz_batch_cnt, support_features, new_xyz, new_xyz_batch_cnt, new_features, new_local_xyz,
                        point_cnt_of_grid, grouped_idxs, num_grid_x, num_grid_y, num_grid_z, max_neighbour_distance, use_xyz,
                        num_max_sum_points, nsample, neighbor_type, pooling_type):
    """vector_pool.cpp:116: returns num_cum_sum, the number of grouped_idxs rows the call needs (the one host read)."""
    N, B, M = support_xyz.shape[0], xyz_batch_cnt.shape[0], new_xyz.shape[0]
    num_c_out, num_c_in, num_total_grids = new_features.shape[1], support_features.shape[1], point_cnt_of_grid.shape[1]
    _numel_ok(support_features, N * num_c_in, "support_features"); _numel_ok(new_xyz_batch_cnt, B, "new_xyz_batch_cnt")
    _numel_ok(new_features, M * num_c_out, "new_features"); _numel_ok(new_local_xyz, M * 3 * num_total_grids, "new_local_xyz")
    _numel_ok(point_cnt_of_grid, M * num_total_grids, "point_cnt_of_grid"); _numel_ok(grouped_idxs, num_max_sum_points * 3, "grouped_idxs")
    ptrs = (_chk(support_xyz, "support_xyz", F32), _chk(support_features, "support_features", F32),
            _chk(xyz_batch_cnt, "xyz_batch_cnt", I32), _chk(new_xyz, "new_xyz", F32), _chk(new_xyz_batch_cnt, "new_xyz_batch_cnt", I32),
            _chk(new_features, "new_features", F32), _chk(new_local_xyz, "new_local_xyz", F32),
            _chk(point_cnt_of_grid, "point_cnt_of_grid", I32), _chk(grouped_idxs, "grouped_idxs", I32))
    total = torch.zeros(1, dtype=I32, device=support_xyz.device)
    _call("pda_stack_vector_pool", support_xyz, *ptrs, total.data_ptr(), B, M, num_c_in, num_c_out, num_total_grids, num_grid_x,
          num_grid_y, num_grid_z, float(max_neighbour_distance), int(use_xyz), num_max_sum_points, nsample, neighbor_type,
          pooling_type)
    return int(total.item())


def vector_pool_grad_wrapper(grad_new_features, point_cnt_of_grid, grouped_idxs, grad_support_features):
    """vector_pool.cpp:173: grad_support_features (N, C_in) zero-filled by the caller."""
    M, num_c_out = grad_new_features.shape[0], grad_new_features.shape[1]
    N, num_c_in = grad_support_features.shape[0], grad_support_features.shape[1]
    num_total_grids, num_max_sum_points = point_cnt_of_grid.shape[1], grouped_idxs.shape[0]
    _numel_ok(point_cnt_of_grid, M * num_total_grids, "point_cnt_of_grid")
    _call("pda_stack_vector_pool_grad", grad_new_features, _chk(grad_new_features, "grad_new_features", F32),
          _chk(point_cnt_of_grid, "point_cnt_of_grid", I32), _chk(grouped_idxs, "grouped_idxs", I32),
          _chk(grad_support_features, "grad_support_features", F32), N, M, num_c_out, num_c_in, num_total_grids, num_max_sum_points)
    return 1
