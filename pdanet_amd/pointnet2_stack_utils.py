"""Mirror of pcdet/ops/pointnet2/pointnet2_stack/pointnet2_utils.py:1-448 (BallQuery, GroupingOperation,
QueryAndGroup, FarthestPointSampling, StackFarthestPointSampling, ThreeNN, ThreeInterpolate,
ThreeNNForVectorPoolByTwoStep, VectorPoolWithVoxelQuery) and voxel_query_utils.py:10-100 (VoxelQuery,
VoxelQueryAndGrouping) over pdanet_amd.pointnet2_stack_cuda.  Allocation contracts as in the reference (idx zero-filled, temp = 1e10,
grads zero-filled); `torch.cuda.IntTensor(...)` constructors replaced by device-aware factories."""
import torch
import torch.nn as nn
from torch.autograd import Function

from . import pointnet2_stack_cuda as pointnet2


class BallQuery(Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
        """xyz (N1+N2..., 3), new_xyz (M1+M2..., 3) -> idx (M, nsample) local indices, empty_ball_mask (M)."""
        assert new_xyz.is_contiguous() and new_xyz_batch_cnt.is_contiguous() and xyz.is_contiguous() and xyz_batch_cnt.is_contiguous()
        B, M = xyz_batch_cnt.shape[0], new_xyz.shape[0]
        idx = torch.zeros((M, nsample), dtype=torch.int32, device=xyz.device)
        pointnet2.ball_query_wrapper(B, M, radius, nsample, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, idx)
        empty_ball_mask = (idx[:, 0] == -1)
        idx[empty_ball_mask] = 0
        ctx.mark_non_differentiable(idx, empty_ball_mask)
        return idx, empty_ball_mask

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None, None, None, None, None


ball_query = BallQuery.apply


class GroupingOperation(Function):
    @staticmethod
    def forward(ctx, features, features_batch_cnt, idx, idx_batch_cnt):
        """features (N, C), idx (M, nsample) -> (M, C, nsample)."""
        assert features.is_contiguous() and features_batch_cnt.is_contiguous() and idx.is_contiguous() and idx_batch_cnt.is_contiguous()
        M, nsample = idx.size()
        N, C = features.size()
        B = idx_batch_cnt.shape[0]
        output = torch.empty((M, C, nsample), dtype=torch.float32, device=features.device)
        pointnet2.group_points_wrapper(B, M, C, nsample, features, features_batch_cnt, idx, idx_batch_cnt, output)
        ctx.for_backwards = (B, N, idx, features_batch_cnt, idx_batch_cnt)
        return output

    @staticmethod
    def backward(ctx, grad_out):
        B, N, idx, features_batch_cnt, idx_batch_cnt = ctx.for_backwards
        M, C, nsample = grad_out.size()
        grad_features = torch.zeros((N, C), dtype=torch.float32, device=grad_out.device)
        pointnet2.group_points_grad_wrapper(B, M, C, N, nsample, grad_out.contiguous(), idx, idx_batch_cnt,
                                            features_batch_cnt, grad_features)
        return grad_features, None, None, None


grouping_operation = GroupingOperation.apply


class QueryAndGroup(nn.Module):
    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None):
        """-> new_features (M, 3 + C, nsample), idx (pointnet2_utils.py:113-158)."""
        idx, empty_ball_mask = ball_query(self.radius, self.nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
        grouped_xyz = grouping_operation(xyz, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        grouped_xyz = grouped_xyz - new_xyz.unsqueeze(-1)
        grouped_xyz = grouped_xyz.masked_fill(empty_ball_mask[:, None, None], 0)
        if features is not None:
            grouped_features = grouping_operation(features, xyz_batch_cnt, idx, new_xyz_batch_cnt)
            grouped_features = grouped_features.masked_fill(empty_ball_mask[:, None, None], 0)
            new_features = torch.cat([grouped_xyz, grouped_features], dim=1) if self.use_xyz else grouped_features
        else:
            assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
            new_features = grouped_xyz
        return new_features, idx


class FarthestPointSampling(Function):
    @staticmethod
    def forward(ctx, xyz, npoint):
        assert xyz.is_contiguous()
        B, N, _ = xyz.size()
        output = torch.empty((B, npoint), dtype=torch.int32, device=xyz.device)
        temp = torch.full((B, N), 1e10, dtype=torch.float32, device=xyz.device)
        pointnet2.farthest_point_sampling_wrapper(B, N, npoint, xyz, temp, output)
        ctx.mark_non_differentiable(output)
        return output

    @staticmethod
    def backward(ctx, a=None):
        return None, None


farthest_point_sample = furthest_point_sample = FarthestPointSampling.apply


class StackFarthestPointSampling(Function):
    @staticmethod
    def forward(ctx, xyz, xyz_batch_cnt, npoint):
        """xyz (N1+N2..., 3); npoint int, list or int tensor -> (sum npoint) global indices (:186-216)."""
        assert xyz.is_contiguous() and xyz.shape[1] == 3
        batch_size = len(xyz_batch_cnt)
        if not isinstance(npoint, torch.Tensor):
            if not isinstance(npoint, list):
                npoint = [npoint for _ in range(batch_size)]
            total = int(sum(npoint))
            npoint = torch.tensor(npoint, device=xyz.device).int()
        else:
            total = int(npoint.sum().item())
        temp = torch.full((xyz.shape[0],), 1e10, dtype=torch.float32, device=xyz.device)
        output = torch.empty((total,), dtype=torch.int32, device=xyz.device)
        pointnet2.stack_farthest_point_sampling_wrapper(xyz, temp, xyz_batch_cnt, output, npoint)
        ctx.mark_non_differentiable(output)
        return output

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None


stack_farthest_point_sample = StackFarthestPointSampling.apply


class ThreeNN(Function):
    @staticmethod
    def forward(ctx, unknown, unknown_batch_cnt, known, known_batch_cnt):
        """-> dist (N, 3) l2 distances, idx (N, 3) global indices of the 3 nearest known points."""
        assert unknown.dim() == 2 and unknown.shape[1] == 3 and known.dim() == 2 and known.shape[1] == 3
        assert len(unknown_batch_cnt) == len(known_batch_cnt)
        dist2 = unknown.new_zeros(unknown.shape)
        idx = unknown_batch_cnt.new_zeros(unknown.shape).int()
        pointnet2.three_nn_wrapper(unknown.contiguous(), unknown_batch_cnt.contiguous(), known.contiguous(),
                                   known_batch_cnt.contiguous(), dist2, idx)
        ctx.mark_non_differentiable(idx)
        return torch.sqrt(dist2), idx

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None, None, None


three_nn = ThreeNN.apply


class ThreeInterpolate(Function):
    @staticmethod
    def forward(ctx, features, idx, weight):
        """features (M, C), idx / weight (N, 3) -> (N, C)."""
        assert idx.shape[0] == weight.shape[0] and idx.shape[1] == weight.shape[1] == 3
        ctx.three_interpolate_for_backward = (idx, weight, features.shape[0])
        output = features.new_zeros((idx.shape[0], features.shape[1]))
        pointnet2.three_interpolate_wrapper(features.contiguous(), idx.contiguous(), weight.contiguous(), output)
        return output

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight, M = ctx.three_interpolate_for_backward
        grad_features = grad_out.new_zeros((M, grad_out.shape[1]))
        pointnet2.three_interpolate_grad_wrapper(grad_out.contiguous(), idx.contiguous(), weight.contiguous(), grad_features)
        return grad_features, None, None


three_interpolate = ThreeInterpolate.apply


class VoxelQuery(Function):
    @staticmethod
    def forward(ctx, max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices):
        """new_coords (M, 4) [batch, z, y, x], point_indices (B, Z, Y, X) -> idx (M, nsample) GLOBAL rows of xyz,
        empty_ball_mask (M) (voxel_query_utils.py:13-42)."""
        assert new_xyz.is_contiguous() and xyz.is_contiguous() and new_coords.is_contiguous() and point_indices.is_contiguous()
        M = new_coords.shape[0]
        B, Z, Y, X = point_indices.shape
        idx = torch.zeros((M, nsample), dtype=torch.int32, device=xyz.device)
        z_range, y_range, x_range = max_range
        pointnet2.voxel_query_wrapper(M, Z, Y, X, nsample, radius, z_range, y_range, x_range, new_xyz, xyz, new_coords,
                                      point_indices, idx)
        empty_ball_mask = (idx[:, 0] == -1)
        idx[empty_ball_mask] = 0
        ctx.mark_non_differentiable(idx, empty_ball_mask)
        return idx, empty_ball_mask

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None, None, None, None, None, None


voxel_query = VoxelQuery.apply


class VoxelQueryAndGrouping(nn.Module):
    def __init__(self, max_range, radius, nsample):
        super().__init__()
        self.max_range, self.radius, self.nsample = max_range, radius, nsample

    def forward(self, new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, voxel2point_indices):
        """-> grouped_features (M, C, nsample), grouped_xyz (M, 3, nsample), empty_ball_mask (M)
        (voxel_query_utils.py:61-100).  The reference subtracts each scene's start in a Python loop over
        idx.view(batch_size, -1, nsample), which reads the counts on the host and needs equally many centres per scene;
        here every centre subtracts the start of its own scene, found on the device."""
        idx, empty_ball_mask = voxel_query(self.max_range, self.radius, self.nsample, xyz, new_xyz, new_coords, voxel2point_indices)
        centre_end = torch.cumsum(new_xyz_batch_cnt, 0)
        scene = torch.searchsorted(centre_end, torch.arange(idx.shape[0], device=idx.device), right=True)
        scene = scene.clamp_(max=xyz_batch_cnt.shape[0] - 1)
        xyz_start = torch.cumsum(xyz_batch_cnt, 0) - xyz_batch_cnt
        idx = (idx - xyz_start[scene].to(idx.dtype)[:, None]).masked_fill_(empty_ball_mask[:, None], 0).contiguous()
        grouped_xyz = grouping_operation(xyz, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        grouped_features = grouping_operation(features, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        return grouped_features, grouped_xyz, empty_ball_mask


class ThreeNNForVectorPoolByTwoStep(Function):
    @staticmethod
    def forward(ctx, support_xyz, xyz_batch_cnt, new_xyz, new_xyz_grid_centers, new_xyz_batch_cnt, max_neighbour_distance,
                nsample, neighbor_type, avg_length_of_neighbor_idxs, num_total_grids, neighbor_distance_multiplier):
        """new_xyz_grid_centers (M, num_total_grids, 3) -> dist (M, G, 3), idx (M, G, 3) GLOBAL rows of support_xyz or -1,
        and the list length per centre that fitted, for the next call (pointnet2_utils.py:302-351)."""
        num_new_xyz = new_xyz.shape[0]
        new_xyz_grid_dist2 = new_xyz_grid_centers.new_zeros(new_xyz_grid_centers.shape)
        new_xyz_grid_idxs = torch.full(new_xyz_grid_centers.shape, -1, dtype=torch.int32, device=new_xyz_grid_centers.device)
        while True:
            num_max_sum_points = avg_length_of_neighbor_idxs * num_new_xyz
            stack_neighbor_idxs = new_xyz_grid_idxs.new_zeros(num_max_sum_points)
            start_len = new_xyz_grid_idxs.new_zeros((num_new_xyz, 2))
            cumsum = new_xyz_grid_idxs.new_zeros(1)
            pointnet2.query_stacked_local_neighbor_idxs_wrapper_stack(
                support_xyz.contiguous(), xyz_batch_cnt.contiguous(), new_xyz.contiguous(), new_xyz_batch_cnt.contiguous(),
                stack_neighbor_idxs, start_len, cumsum, avg_length_of_neighbor_idxs,
                max_neighbour_distance * neighbor_distance_multiplier, nsample, neighbor_type)
            total = int(cumsum[0].item())
            avg_length_of_neighbor_idxs = total // num_new_xyz + int(total % num_new_xyz > 0) if num_new_xyz > 0 else 0
            if total <= num_max_sum_points:
                break
        stack_neighbor_idxs = stack_neighbor_idxs[:total]
        pointnet2.query_three_nn_by_stacked_local_idxs_wrapper_stack(
            support_xyz.contiguous(), new_xyz.contiguous(), new_xyz_grid_centers.contiguous(), new_xyz_grid_idxs,
            new_xyz_grid_dist2, stack_neighbor_idxs, start_len, num_new_xyz, num_total_grids)
        dist, avg = torch.sqrt(new_xyz_grid_dist2), torch.tensor(avg_length_of_neighbor_idxs)
        ctx.mark_non_differentiable(dist, new_xyz_grid_idxs, avg)
        return dist, new_xyz_grid_idxs, avg

    @staticmethod
    def backward(ctx, a=None, b=None, c=None):
        return (None,) * 11


three_nn_for_vector_pool_by_two_step = ThreeNNForVectorPoolByTwoStep.apply


class VectorPoolWithVoxelQuery(Function):
    @staticmethod
    def forward(ctx, support_xyz, xyz_batch_cnt, support_features, new_xyz, new_xyz_batch_cnt, num_grid_x, num_grid_y,
                num_grid_z, max_neighbour_distance, num_c_out_each_grid, use_xyz, num_mean_points_per_grid=100, nsample=-1,
                neighbor_type=0, pooling_type=0):
        """support_features (N, C_in) -> new_features (M, num_total_grids * num_c_out_each_grid) means per cell,
        new_local_xyz (M, 3 * num_total_grids), num_mean_points_per_grid that fitted, point_cnt_of_grid (M, num_total_grids)
        (pointnet2_utils.py:357-425)."""
        assert support_xyz.is_contiguous() and support_features.is_contiguous() and xyz_batch_cnt.is_contiguous()
        assert new_xyz.is_contiguous() and new_xyz_batch_cnt.is_contiguous()
        num_total_grids = num_grid_x * num_grid_y * num_grid_z
        num_c_out = num_c_out_each_grid * num_total_grids
        N, num_c_in = support_features.shape
        M = new_xyz.shape[0]
        assert num_c_in % num_c_out_each_grid == 0, \
            f'the input channels ({num_c_in}) should be an integral multiple of num_c_out_each_grid({num_c_out_each_grid})'
        while True:
            new_features = support_features.new_zeros((M, num_c_out))
            new_local_xyz = support_features.new_zeros((M, 3 * num_total_grids))
            point_cnt_of_grid = xyz_batch_cnt.new_zeros((M, num_total_grids))
            num_max_sum_points = num_mean_points_per_grid * M
            grouped_idxs = xyz_batch_cnt.new_zeros((num_max_sum_points, 3))
            num_cum_sum = pointnet2.vector_pool_wrapper(
                support_xyz, xyz_batch_cnt, support_features, new_xyz, new_xyz_batch_cnt, new_features, new_local_xyz,
                point_cnt_of_grid, grouped_idxs, num_grid_x, num_grid_y, num_grid_z, max_neighbour_distance, use_xyz,
                num_max_sum_points, nsample, neighbor_type, pooling_type)
            num_mean_points_per_grid = num_cum_sum // M + int(num_cum_sum % M > 0) if M > 0 else 0
            if num_cum_sum <= num_max_sum_points:
                break
        grouped_idxs = grouped_idxs[:num_cum_sum]
        normalizer = torch.clamp_min(point_cnt_of_grid[:, :, None].float(), min=1e-6)
        new_features = (new_features.view(-1, num_total_grids, num_c_out_each_grid) / normalizer).view(-1, num_c_out)
        if use_xyz:
            new_local_xyz = (new_local_xyz.view(-1, num_total_grids, 3) / normalizer).view(-1, num_total_grids * 3)
        num_mean_points_per_grid = torch.tensor([num_mean_points_per_grid], dtype=torch.int32)
        ctx.vector_pool_for_backward = (point_cnt_of_grid, grouped_idxs, N, num_c_in)
        ctx.mark_non_differentiable(new_local_xyz, num_mean_points_per_grid, point_cnt_of_grid)
        return new_features, new_local_xyz, num_mean_points_per_grid, point_cnt_of_grid

    @staticmethod
    def backward(ctx, grad_new_features, grad_local_xyz=None, grad_num_cum_sum=None, grad_point_cnt_of_grid=None):
        point_cnt_of_grid, grouped_idxs, N, num_c_in = ctx.vector_pool_for_backward
        grad_support_features = grad_new_features.new_zeros((N, num_c_in))
        pointnet2.vector_pool_grad_wrapper(grad_new_features.contiguous(), point_cnt_of_grid, grouped_idxs, grad_support_features)
        return (None, None, grad_support_features) + (None,) * 12


vector_pool_with_voxel_query_op = VectorPoolWithVoxelQuery.apply
