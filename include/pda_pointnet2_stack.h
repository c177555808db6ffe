/* pda_pointnet2_stack.h -- C ABI of the pointnet2_stack operator set
 * (/root/reference/pcdet/ops/pointnet2/pointnet2_stack/src/pointnet2_api.cpp:12-31): scenes of different
 * sizes stacked along the point axis and described by int32 *_batch_cnt arrays (device memory), features
 * point-major (N, C).  Same library and conventions as pda_pointnet2.h.  All fourteen entry points of that module
 * are covered; its batch-layout farthest_point_sampling_wrapper (:16) is pda_furthest_point_sampling.
 */
#ifndef PDA_POINTNET2_STACK_H
#define PDA_POINTNET2_STACK_H
#include "pda_pointnet2.h"

#ifdef __cplusplus
extern "C" {
#endif

/* replaces ball_query_wrapper_stack (ball_query.cpp:22-40 -> ball_query_gpu.cu:16-66): new_xyz (M,3),
 * xyz (N,3) -> idx (M,nsample) indices LOCAL to the centre's scene, first hit pre-fills the row, a ball
 * with no hit gets idx[0] = -1 and is otherwise untouched (caller zero-fills, pointnet2_utils.py:32). */
int pda_stack_ball_query(const float *new_xyz, const int32_t *new_xyz_batch_cnt, const float *xyz,
                         const int32_t *xyz_batch_cnt, int32_t *idx, int b, int m, float radius,
                         int nsample, pda_stream_t stream);
/* replace group_points_wrapper_stack / group_points_grad_wrapper_stack (group_points.cpp:41-68 / :19-38 ->
 * group_points_gpu.cu:71-102 / :15-45): features (N,C), idx (M,nsample) local -> out (M,C,nsample);
 * grad_features (N,C) pre-zeroed, accumulated with atomics. */
int pda_stack_group_points(const float *features, const int32_t *features_batch_cnt, const int32_t *idx,
                           const int32_t *idx_batch_cnt, float *out, int b, int m, int c, int nsample,
                           pda_stream_t stream);
int pda_stack_group_points_grad(const float *grad_out, const int32_t *idx, const int32_t *idx_batch_cnt,
                                const int32_t *features_batch_cnt, float *grad_features, int b, int m,
                                int c, int n, int nsample, pda_stream_t stream);
/* replaces stack_farthest_point_sampling_wrapper (sampling.cpp:38-58 -> sampling_gpu.cu:188-345): xyz (N,3),
 * temp (N) pre-filled 1e10, num_sampled_points (B) -> idx (sum of num_sampled_points) GLOBAL indices;
 * the reference's fixed block size 1024 fixes the tie-break order. */
int pda_stack_furthest_point_sampling(const float *xyz, float *temp, const int32_t *xyz_batch_cnt,
                                      int32_t *idx, const int32_t *num_sampled_points, int b,
                                      pda_stream_t stream);
/* replaces three_nn_wrapper_stack (interpolate.cpp:24-47 -> interpolate_gpu.cu:16-99): unknown (N,3),
 * known (M,3) -> dist2 (N,3) squared distances, idx (N,3) GLOBAL known indices. */
int pda_stack_three_nn(const float *unknown, const int32_t *unknown_batch_cnt, const float *known,
                       const int32_t *known_batch_cnt, float *dist2, int32_t *idx, int b, int n,
                       pda_stream_t stream);
/* replace three_interpolate_wrapper_stack / three_interpolate_grad_wrapper_stack (interpolate.cpp:50-107 ->
 * interpolate_gpu.cu:107-189): features (M,C), idx / weight (N,3) -> out (N,C); grad_features (M,C) pre-zeroed. */
int pda_stack_three_interpolate(const float *features, const int32_t *idx, const float *weight, float *out,
                                int n, int c, pda_stream_t stream);
int pda_stack_three_interpolate_grad(const float *grad_out, const int32_t *idx, const float *weight,
                                     float *grad_features, int n, int c, pda_stream_t stream);

/* replaces voxel_query_wrapper_stack (voxel_query.cpp:28-44 -> voxel_query_gpu.cu:10-89): new_xyz (M,3), xyz (N,3),
 * new_coords (M,4) [batch, z, y, x], point_indices (B,R1,R2,R3) point of each voxel or < 0 -> idx (M,nsample) GLOBAL
 * rows of xyz.  Cells are walked dz, dy, dx over [-range, +range] clipped to the grid, a point is accepted when
 * dist2 <= radius^2, the first hit pre-fills the row, an empty ball gets idx[0] = -1 and is otherwise untouched.
 * A batch index outside [0, b) or a cell entry >= n is skipped instead of read. */
int pda_stack_voxel_query(const float *new_xyz, const float *xyz, const int32_t *new_coords,
                          const int32_t *point_indices, int32_t *idx, int b, int n, int m, int r1, int r2,
                          int r3, int nsample, float radius, int z_range, int y_range, int x_range,
                          pda_stream_t stream);
/* replaces query_stacked_local_neighbor_idxs_wrapper_stack (vector_pool.cpp:35-75 -> vector_pool_gpu.cu:122-205):
 * per centre the ascending indices of its scene's points inside the ball (neighbor_type 1, dist2 <= d^2) or the
 * cube (every |local| <= d), at most nsample (when > 0) and never more than 1000.  start_len (M,2) = [start, count];
 * rows are written as GLOBAL indices at stack_neighbor_idxs[start ...], cut at avg_length_of_neighbor_idxs * M;
 * cumsum[0] (pre-zeroed) grows by the total.  Starts follow the centre order (a scan, not the reference's atomic
 * counter), so two calls give the same bits. */
int pda_stack_query_local_neighbor_idxs(const float *support_xyz, const int32_t *xyz_batch_cnt,
                                        const float *new_xyz, const int32_t *new_xyz_batch_cnt,
                                        int32_t *stack_neighbor_idxs, int32_t *start_len, int32_t *cumsum,
                                        int avg_length_of_neighbor_idxs, float max_neighbour_distance, int b,
                                        int m, int nsample, int neighbor_type, pda_stream_t stream);
/* replaces query_three_nn_by_stacked_local_idxs_wrapper_stack (vector_pool.cpp:78-113 -> vector_pool_gpu.cu:19-86):
 * new_xyz_grid_centers (M,G,3) -> new_xyz_grid_idxs / new_xyz_grid_dist2 (M,G,3): the three nearest entries of the
 * centre's list (strict <, list order), a missing second or third repeats the first, an empty list gives -1 / inf.
 * num_neighbor_idxs is the length of stack_neighbor_idxs: a list that reaches past it is read up to it only. */
int pda_stack_three_nn_by_local_idxs(const float *support_xyz, const float *new_xyz_grid_centers,
                                     int32_t *new_xyz_grid_idxs, float *new_xyz_grid_dist2,
                                     const int32_t *stack_neighbor_idxs, const int32_t *start_len, int n,
                                     int64_t num_neighbor_idxs, int m, int num_total_grids, pda_stream_t stream);
/* replaces vector_pool_wrapper_stack (vector_pool.cpp:116-170 -> vector_pool_gpu.cu:243-430): support_features (N,C_in)
 * -> new_features (M,C_out) raw sums, new_local_xyz (M,3G), point_cnt_of_grid (M,G), grouped_idxs
 * (num_max_sum_points,3) rows [global k, centre, cell] in no defined order; all four pre-zeroed by the caller.
 * pooling_type 0 sums every hit, 1 takes the first point of each cell.  num_cum_sum is one int32 in device (or
 * pinned) memory: the entry zeroes it and the kernel leaves the number of rows the call needs there; when it exceeds
 * num_max_sum_points the caller retries with more rows and every other output of this call is unspecified. */
int pda_stack_vector_pool(const float *support_xyz, const float *support_features, const int32_t *xyz_batch_cnt,
                          const float *new_xyz, const int32_t *new_xyz_batch_cnt, float *new_features,
                          float *new_local_xyz, int32_t *point_cnt_of_grid, int32_t *grouped_idxs,
                          int32_t *num_cum_sum, int b, int m, int c_in, int c_out, int num_total_grids,
                          int num_grid_x, int num_grid_y, int num_grid_z, float max_neighbour_distance,
                          int use_xyz, int num_max_sum_points, int nsample, int neighbor_type, int pooling_type,
                          pda_stream_t stream);
/* replaces vector_pool_grad_wrapper_stack (vector_pool.cpp:173-203 -> vector_pool_gpu.cu:433-486): per grouped_idxs
 * row and input channel grad_support_features[k, c] += grad_new_features[centre, cell * ce + c % ce] / max(count, 1);
 * grad_support_features (N,C_in) pre-zeroed, accumulated with atomics. */
int pda_stack_vector_pool_grad(const float *grad_new_features, const int32_t *point_cnt_of_grid,
                               const int32_t *grouped_idxs, float *grad_support_features, int n, int m,
                               int c_out, int c_in, int num_total_grids, int num_max_sum_points,
                               pda_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
