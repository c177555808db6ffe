"""VectorPoolLocalInterpolateModule, VectorPoolAggregationModule and VectorPoolAggregationModuleMSG
(pcdet/ops/pointnet2/pointnet2_stack/pointnet2_modules.py:160-470): the layers of PV-RCNN++'s keypoint encoder and of its
RoI-grid pool, under the reference's constructors, config keys, attribute names (layer_k, separate_local_aggregation_layer,
post_mlps, msg_post_mlps), init_weights and state-dict keys.  The growing length hints (num_avg_length_of_neighbor_idxs,
num_mean_points_per_grid) are kept as the reference keeps them: a call whose lists did not fit runs again with the length
that fits, and the next call starts from the largest length seen.  No config list is modified (the reference adds 9 to mlp[0]
in place).

local_interpolation.  The two-step three-NN (pointnet2_stack_utils.three_nn_for_vector_pool_by_two_step) gives dist and idx
(M, G, 3).  Two paths assemble the rows from them, chosen when the layer runs by PDA_VECTOR_POOL = fused | composed:
  composed  the reference's sequence: weights in torch (the sum of the three reciprocals written out left to right),
            three_interpolate, a gather of the neighbours' coordinates, a concatenation and a masked fill.  The yardstick of
            the tests; the fused forward gives the same bits.
  fused     pda_vector_interp_fwd / _bwd (csrc/spc_sample.hip), the default with use_xyz: the (M, G * (C + 9)) rows are written
            once; the backward reads the gradient rows in place and adds into a zero-filled grad_support_features with float
            atomics, as the reference's three_interpolate_grad does, so that gradient is not bit-reproducible.  Coordinates
            and grid centres get no gradient on this path (keypoints, voxel centres and RoI grid points carry none).

voxel_avg_pool / voxel_random_choice call pointnet2_stack_utils.vector_pool_with_voxel_query_op; its pooling_type 1 is the
reference's deterministic "first point of a cell".

One host read per call of either kind: the total length of the lists (three-NN) or of grouped_idxs (vector pool)."""
from functools import partial

import torch
import torch.nn as nn

from . import pointnet2_stack_modules
from . import pointnet2_stack_utils as pointnet2_utils
from .config import fused_or_composed
from .pointnet2_batch_cuda import F32, I32, _call, _chk

# 'fused' (default) or 'composed', read when a layer runs
ENV = "PDA_VECTOR_POOL"
interp_path = partial(fused_or_composed, ENV)


class _VectorInterp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, support_features, dist, idx, support_xyz, grid_centers):
        M, G = idx.shape[0], idx.shape[1]
        N, C = support_features.shape
        support_features = support_features.contiguous()
        out = torch.empty((M, G * (C + 9)), dtype=F32, device=support_features.device)
        _call("pda_vector_interp_fwd", support_features, _chk(dist, "dist", F32), _chk(idx, "idx", I32),
              _chk(support_xyz, "support_xyz", F32), _chk(support_features, "support_features", F32),
              _chk(grid_centers, "grid_centers", F32), out.data_ptr(), M, G, N, C)
        ctx.save_for_backward(dist, idx)
        ctx.shape = (M, G, N, C)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        dist, idx = ctx.saved_tensors
        M, G, N, C = ctx.shape
        grad_out = grad_out.contiguous()
        grad_features = torch.zeros((N, C), dtype=F32, device=grad_out.device)
        _call("pda_vector_interp_bwd", grad_out, _chk(grad_out, "grad_out", F32), _chk(dist, "dist", F32), _chk(idx, "idx", I32),
              grad_features.data_ptr(), M, G, N, C)
        return grad_features, None, None, None, None


def vector_interp(support_features, dist, idx, support_xyz, grid_centers):
    """support_features (N, C), dist / idx (M, G, 3) of the two-step three-NN (idx[..., 0] == -1: no neighbour), support_xyz
    (N, 3), grid_centers (M, G, 3) -> (M, G * (C + 9)): per cell the inverse-distance blend of three feature rows and the nine
    coordinates grid centre - neighbour, zeros for a cell without neighbour.  The gradient reaches support_features only; it is
    added with float atomics, as the reference's three_interpolate_grad adds it, and is not bit-reproducible."""
    return _VectorInterp.apply(support_features, dist.contiguous(), idx.contiguous(), support_xyz.detach().contiguous(),
                               grid_centers.detach().contiguous())


def _conv_bn_relu(conv, channels):
    layers = []
    for k in range(len(channels) - 1):
        layers.extend([conv(channels[k], channels[k + 1], kernel_size=1, bias=False),
                       (nn.BatchNorm2d if conv is nn.Conv2d else nn.BatchNorm1d)(channels[k + 1]), nn.ReLU()])
    return nn.Sequential(*layers)


class VectorPoolLocalInterpolateModule(nn.Module):
    def __init__(self, mlp, num_voxels, max_neighbour_distance, nsample, neighbor_type, use_xyz=True,
                 neighbour_distance_multiplier=1.0, xyz_encoding_type='concat'):
        """num_voxels: the cells of the local grid around a centre; neighbor_type 1: ball, others: cube; nsample -1: all."""
        super().__init__()
        if xyz_encoding_type != 'concat':
            raise NotImplementedError("xyz_encoding_type %r" % (xyz_encoding_type,))
        self.num_voxels = num_voxels
        self.num_total_grids = self.num_voxels[0] * self.num_voxels[1] * self.num_voxels[2]
        self.max_neighbour_distance = max_neighbour_distance
        self.neighbor_distance_multiplier = neighbour_distance_multiplier
        self.nsample = nsample
        self.neighbor_type = neighbor_type
        self.use_xyz = use_xyz
        self.xyz_encoding_type = xyz_encoding_type
        if mlp is not None:
            mlp = list(mlp)                             # a copy: the caller's list stays as it is
            if self.use_xyz:
                mlp[0] += 9
            self.mlp = _conv_bn_relu(nn.Conv2d, mlp)
        else:
            self.mlp = None
        self.num_avg_length_of_neighbor_idxs = 1000

    def _rows_composed(self, support_xyz, support_features, new_xyz_grid_centers, dist, idx):
        """pointnet2_modules.py:220-238"""
        dist_recip = 1.0 / (dist + 1e-8)
        # left to right: torch.sum leaves the association of its three terms to the device's reduction (on an MI355X it is neither
        # (a + b) + c nor a + (b + c)), and the fused kernel has to add in the same order to give the same bits
        norm = (dist_recip[..., 0:1] + dist_recip[..., 1:2]) + dist_recip[..., 2:3]
        weight = dist_recip / torch.clamp_min(norm, min=1e-8)
        empty_mask = (idx.view(-1, 3)[:, 0] == -1)
        idx = idx.view(-1, 3).masked_fill(empty_mask[:, None], 0)
        feats = pointnet2_utils.three_interpolate(support_features, idx, weight.view(-1, 3))
        if self.use_xyz:
            near_known_xyz = support_xyz[idx.long()].view(-1, 3, 3)
            local_xyz = (new_xyz_grid_centers.view(-1, 1, 3) - near_known_xyz).view(-1, 9)
            feats = torch.cat((feats, local_xyz), dim=-1)
        return feats.masked_fill(empty_mask[:, None], 0)

    def forward(self, support_xyz, support_features, xyz_batch_cnt, new_xyz, new_xyz_grid_centers, new_xyz_batch_cnt):
        """support_xyz (N1 + N2 ..., 3), support_features (N, C), new_xyz (M1 + M2 ..., 3), new_xyz_grid_centers
        (M, num_total_grids, 3), the int32 counts per scene -> (M * num_total_grids, C + 9), or the mlp's width."""
        with torch.no_grad():
            dist, idx, avg = pointnet2_utils.three_nn_for_vector_pool_by_two_step(
                support_xyz, xyz_batch_cnt, new_xyz, new_xyz_grid_centers, new_xyz_batch_cnt, self.max_neighbour_distance,
                self.nsample, self.neighbor_type, self.num_avg_length_of_neighbor_idxs, self.num_total_grids,
                self.neighbor_distance_multiplier)
        self.num_avg_length_of_neighbor_idxs = max(self.num_avg_length_of_neighbor_idxs, avg.item())
        if interp_path() == "fused" and self.use_xyz:
            rows = vector_interp(support_features, dist, idx, support_xyz, new_xyz_grid_centers)
            new_features = rows.view(-1, support_features.shape[1] + 9)
        else:
            new_features = self._rows_composed(support_xyz, support_features, new_xyz_grid_centers, dist, idx)
        if self.mlp is not None:
            new_features = self.mlp(new_features.permute(1, 0)[None, :, :, None])
            new_features = new_features.squeeze(dim=0).squeeze(dim=-1).permute(1, 0)
        return new_features


class VectorPoolAggregationModule(nn.Module):
    def __init__(self, input_channels, num_local_voxel=(3, 3, 3), local_aggregation_type='local_interpolation',
                 num_reduced_channels=30, num_channels_of_local_aggregation=32, post_mlps=(128,), max_neighbor_distance=None,
                 neighbor_nsample=-1, neighbor_type=0, neighbor_distance_multiplier=2.0):
        super().__init__()
        self.num_local_voxel = num_local_voxel
        self.total_voxels = self.num_local_voxel[0] * self.num_local_voxel[1] * self.num_local_voxel[2]
        self.local_aggregation_type = local_aggregation_type
        assert self.local_aggregation_type in ['local_interpolation', 'voxel_avg_pool', 'voxel_random_choice']
        self.input_channels = input_channels
        self.num_reduced_channels = input_channels if num_reduced_channels is None else num_reduced_channels
        self.num_channels_of_local_aggregation = num_channels_of_local_aggregation
        self.max_neighbour_distance = max_neighbor_distance
        self.neighbor_nsample = neighbor_nsample
        self.neighbor_type = neighbor_type              # 1: ball, others: cube

        if self.local_aggregation_type == 'local_interpolation':
            self.local_interpolate_module = VectorPoolLocalInterpolateModule(
                mlp=None, num_voxels=self.num_local_voxel, max_neighbour_distance=self.max_neighbour_distance,
                nsample=self.neighbor_nsample, neighbor_type=self.neighbor_type,
                neighbour_distance_multiplier=neighbor_distance_multiplier)
            num_c_in = (self.num_reduced_channels + 9) * self.total_voxels
        else:
            self.local_interpolate_module = None
            num_c_in = (self.num_reduced_channels + 3) * self.total_voxels
        num_c_out = self.total_voxels * self.num_channels_of_local_aggregation

        self.separate_local_aggregation_layer = nn.Sequential(
            nn.Conv1d(num_c_in, num_c_out, kernel_size=1, groups=self.total_voxels, bias=False),
            nn.BatchNorm1d(num_c_out), nn.ReLU())
        self.post_mlps = _conv_bn_relu(nn.Conv1d, [num_c_out] + list(post_mlps))
        self.num_mean_points_per_grid = 20
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def vector_pool_with_voxel_query(self, xyz, xyz_batch_cnt, features, new_xyz, new_xyz_batch_cnt):
        pooling_type = 0 if self.local_aggregation_type == 'voxel_avg_pool' else 1
        new_features, new_local_xyz, num_mean_points_per_grid, point_cnt_of_grid = pointnet2_utils.vector_pool_with_voxel_query_op(
            xyz, xyz_batch_cnt, features, new_xyz, new_xyz_batch_cnt, self.num_local_voxel[0], self.num_local_voxel[1],
            self.num_local_voxel[2], self.max_neighbour_distance, self.num_reduced_channels, 1, self.num_mean_points_per_grid,
            self.neighbor_nsample, self.neighbor_type, pooling_type)
        self.num_mean_points_per_grid = max(self.num_mean_points_per_grid, num_mean_points_per_grid.item())
        num_new_pts = new_features.shape[0]
        new_local_xyz = new_local_xyz.view(num_new_pts, -1, 3)                            # (M, cells, 3)
        new_features = new_features.view(num_new_pts, -1, self.num_reduced_channels)      # (M, cells, C)
        return torch.cat((new_local_xyz, new_features), dim=-1).view(num_new_pts, -1), point_cnt_of_grid

    @staticmethod
    def get_dense_voxels_by_center(point_centers, max_neighbour_distance, num_voxels):
        """point_centers (M, 3) -> the centres of the local grid's cells (M, total_voxels, 3), x slowest."""
        R = max_neighbour_distance
        device = point_centers.device
        grids = [torch.arange(-R + R / n, R - R / n + 1e-5, 2 * R / n, device=device) for n in num_voxels]
        x_offset, y_offset, z_offset = torch.meshgrid(*grids, indexing='ij')
        xyz_offset = torch.cat((x_offset.contiguous().view(-1, 1), y_offset.contiguous().view(-1, 1),
                                z_offset.contiguous().view(-1, 1)), dim=-1)
        return point_centers[:, None, :] + xyz_offset[None, :, :]

    def vector_pool_with_local_interpolate(self, xyz, xyz_batch_cnt, features, new_xyz, new_xyz_batch_cnt):
        """-> (M, total_voxels * (C + 9))"""
        voxel_centers = self.get_dense_voxels_by_center(point_centers=new_xyz, max_neighbour_distance=self.max_neighbour_distance,
                                                        num_voxels=self.num_local_voxel)
        voxel_features = self.local_interpolate_module(
            support_xyz=xyz, support_features=features, xyz_batch_cnt=xyz_batch_cnt, new_xyz=new_xyz,
            new_xyz_grid_centers=voxel_centers, new_xyz_batch_cnt=new_xyz_batch_cnt)
        return voxel_features.contiguous().view(-1, self.total_voxels * voxel_features.shape[-1])

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, **kwargs):
        """xyz (N1 + N2 ..., 3), new_xyz (M1 + M2 ..., 3), the int32 counts per scene, features (N, C) ->
        new_xyz, new_features (M, post_mlps[-1])."""
        N, C = features.shape
        assert C % self.num_reduced_channels == 0, \
            'the input channels (%d) should be an integral multiple of num_reduced_channels(%d)' % (C, self.num_reduced_channels)
        features = features.view(N, -1, self.num_reduced_channels).sum(dim=1)
        if self.local_aggregation_type in ['voxel_avg_pool', 'voxel_random_choice']:
            vector_features, _ = self.vector_pool_with_voxel_query(
                xyz=xyz, xyz_batch_cnt=xyz_batch_cnt, features=features.contiguous(), new_xyz=new_xyz,
                new_xyz_batch_cnt=new_xyz_batch_cnt)
        else:
            vector_features = self.vector_pool_with_local_interpolate(
                xyz=xyz, xyz_batch_cnt=xyz_batch_cnt, features=features, new_xyz=new_xyz, new_xyz_batch_cnt=new_xyz_batch_cnt)
        vector_features = vector_features.permute(1, 0)[None, :, :]                      # (1, cells * C, M)
        new_features = self.post_mlps(self.separate_local_aggregation_layer(vector_features))
        return new_xyz, new_features.squeeze(dim=0).permute(1, 0)


class VectorPoolAggregationModuleMSG(nn.Module):
    def __init__(self, input_channels, config):
        super().__init__()
        self.model_cfg = config
        self.num_groups = config['NUM_GROUPS']
        c_in = 0
        for k in range(self.num_groups):
            cur_config = config['GROUP_CFG_%d' % k]
            setattr(self, 'layer_%d' % k, VectorPoolAggregationModule(
                input_channels=input_channels, num_local_voxel=cur_config['NUM_LOCAL_VOXEL'], post_mlps=cur_config['POST_MLPS'],
                max_neighbor_distance=cur_config['MAX_NEIGHBOR_DISTANCE'], neighbor_nsample=cur_config['NEIGHBOR_NSAMPLE'],
                local_aggregation_type=config['LOCAL_AGGREGATION_TYPE'],
                num_reduced_channels=config.get('NUM_REDUCED_CHANNELS', None),
                num_channels_of_local_aggregation=config['NUM_CHANNELS_OF_LOCAL_AGGREGATION'], neighbor_distance_multiplier=2.0))
            c_in += cur_config['POST_MLPS'][-1]
        c_in += 3                                       # use_xyz
        self.msg_post_mlps = _conv_bn_relu(nn.Conv1d, [c_in] + list(config['MSG_POST_MLPS']))

    def forward(self, **kwargs):
        features_list = []
        for k in range(self.num_groups):
            cur_xyz, cur_features = getattr(self, 'layer_%d' % k)(**kwargs)
            features_list.append(cur_features)
        features = torch.cat([cur_xyz] + features_list, dim=-1)
        new_features = self.msg_post_mlps(features.permute(1, 0)[None, :, :])            # (1, C, M)
        return cur_xyz, new_features.squeeze(dim=0).permute(1, 0)


def build_local_aggregation_module(input_channels, config):
    """-> (layer, its output width): StackSAModuleMSG through pointnet2_stack_modules' builder, VectorPoolAggregationModuleMSG
    here.  The config is read, not modified."""
    if config.get('NAME', 'StackSAModuleMSG') == 'VectorPoolAggregationModuleMSG':
        return VectorPoolAggregationModuleMSG(input_channels=input_channels, config=config), config['MSG_POST_MLPS'][-1]
    return pointnet2_stack_modules.build_local_aggregation_module(input_channels, config)
