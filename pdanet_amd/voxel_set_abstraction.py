"""VoxelSetAbstraction (pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py): the keypoint encoder of PV-RCNN, under the
reference's constructor, config keys, module names (SA_layers, SA_rawpoints, vsa_point_feature_fusion) and state-dict keys.

Built: POINT_SOURCE raw_points | voxel_centers, SAMPLE_METHOD FPS, FEATURES_SOURCE any of bev, raw_points, x_conv1..4.
Refused at construction by this class: SAMPLE_METHOD SPC (sample_points_with_roi / sector_fps) and
FILTER_NEIGHBOR_WITH_ROI; voxel_set_abstraction_spc.py builds both on the hooks named at the top of the class.

Keypoints.  The reference cuts the batch into scenes with boolean masks and samples each in a Python loop.  Here the counts
per scene come from a bincount of the batch column, one stacked FPS launch samples min(N_b, NUM_KEYPOINTS) points of every
scene, and a scene with fewer points repeats its list (keypoint j = sample j mod N_b), which is the reference's rule.  The B
counts are read on the host once per forward (the size of the FPS output depends on them); nothing else is.  The rows of
`points` / `voxel_coords` must be ordered by scene, as the collate functions leave them.

interpolate_from_bev_features is pda_bev_interpolate_fwd / _bwd (csrc/stack_sa.hip): bilinear_interpolate_torch for the whole
batch in one launch.  The map coordinates are the reference's float32 expressions; the backward adds into a zero-filled map
with float atomics, so the gradient of spatial_features is not bit-reproducible.  Keypoints receive no gradient.

The set-abstraction layers are pointnet2_stack_modules.StackSAModuleMSG (fused in csrc/stack_sa.hip); the counts per scene
of every source come from its batch column on the device."""
import torch
import torch.nn as nn

from . import pointnet2_stack_modules
from . import pointnet2_stack_utils
from .pointnet2_batch_cuda import F32, _call, _chk
from .voxel_utils import get_voxel_centers


class _BevInterpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, keypoints, x_idxs, y_idxs, bev):
        B, C, H, W = bev.shape
        M = keypoints.shape[0]
        bev = bev.contiguous()
        out = torch.empty((M, C), dtype=F32, device=bev.device)
        _call("pda_bev_interpolate_fwd", bev, _chk(keypoints, "keypoints", F32), _chk(x_idxs, "x_idxs", F32),
              _chk(y_idxs, "y_idxs", F32), _chk(bev, "bev_features", F32), out.data_ptr(), M, B, C, H, W)
        ctx.save_for_backward(keypoints, x_idxs, y_idxs)
        ctx.shape = (B, C, H, W)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        keypoints, x_idxs, y_idxs = ctx.saved_tensors
        B, C, H, W = ctx.shape
        grad_out = grad_out.contiguous()
        grad_bev = torch.zeros((B, C, H, W), dtype=F32, device=grad_out.device)
        _call("pda_bev_interpolate_bwd", grad_out, _chk(keypoints, "keypoints", F32), _chk(x_idxs, "x_idxs", F32),
              _chk(y_idxs, "y_idxs", F32), _chk(grad_out, "grad_out", F32), grad_bev.data_ptr(), keypoints.shape[0], B, C, H, W)
        return None, None, None, grad_bev


def bev_interpolate(keypoints, x_idxs, y_idxs, bev_features):
    """keypoints (M, 4) [batch, x, y, z], x_idxs / y_idxs (M) map coordinates, bev_features (B, C, H, W) -> (M, C)."""
    return _BevInterpolate.apply(keypoints.detach().contiguous(), x_idxs.detach().contiguous(), y_idxs.detach().contiguous(),
                                 bev_features)


def scene_counts(batch_column, batch_size):
    """Rows per scene, int32, on the device (the batch column may be float or int)."""
    scenes = torch.arange(batch_size, device=batch_column.device)
    return (batch_column.view(-1, 1) == scenes.view(1, -1).to(batch_column.dtype)).sum(dim=0).int()


def sample_keypoints(src_points, batch_indices, batch_size, num_keypoints):
    """src_points (N, 3) ordered by scene, batch_indices (N) -> rows of src_points (B, num_keypoints): per scene the
    farthest-point samples from its first point, repeated when the scene has fewer points than num_keypoints."""
    counts = torch.bincount(batch_indices.long(), minlength=batch_size)[:batch_size]
    picked = [min(int(v), num_keypoints) for v in counts.tolist()]                 # the one host read
    if min(picked) < 1:
        raise ValueError("VoxelSetAbstraction: a scene without points")
    npoint = torch.tensor(picked, dtype=torch.int32).to(src_points.device, non_blocking=True)
    samples = pointnet2_stack_utils.stack_farthest_point_sample(src_points.contiguous(), counts.int().contiguous(), picked).long()
    start = torch.cumsum(npoint, 0) - npoint
    slot = torch.arange(num_keypoints, device=src_points.device)[None, :] % npoint[:, None]
    return samples[(start[:, None] + slot).long()]


class VoxelSetAbstraction(nn.Module):
    # what voxel_set_abstraction_spc.py (PV-RCNN++) widens: the sampling methods taken, whether a source may ask for
    # FILTER_NEIGHBOR_WITH_ROI, the builder of the layers; and the two methods keypoints_and_counts / source_rows below
    SAMPLE_METHODS = ('FPS',)
    NEIGHBOR_FILTER = False
    build_local_aggregation_module = staticmethod(pointnet2_stack_modules.build_local_aggregation_module)

    def __init__(self, model_cfg, voxel_size, point_cloud_range, num_bev_features=None, num_rawpoint_features=None, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        if model_cfg['SAMPLE_METHOD'] not in self.SAMPLE_METHODS:
            raise NotImplementedError("SAMPLE_METHOD %r (SPC is PV-RCNN++)" % (model_cfg['SAMPLE_METHOD'],))
        if model_cfg['POINT_SOURCE'] not in ('raw_points', 'voxel_centers'):
            raise NotImplementedError("POINT_SOURCE %r" % (model_cfg['POINT_SOURCE'],))
        SA_cfg = model_cfg['SA_LAYER']
        for src_name in model_cfg['FEATURES_SOURCE']:
            if src_name not in ('bev', 'raw_points', 'x_conv1', 'x_conv2', 'x_conv3', 'x_conv4'):
                raise NotImplementedError("FEATURES_SOURCE %r" % (src_name,))
            if src_name != 'bev' and SA_cfg[src_name].get('FILTER_NEIGHBOR_WITH_ROI', False) and not self.NEIGHBOR_FILTER:
                raise NotImplementedError("FILTER_NEIGHBOR_WITH_ROI (PV-RCNN++)")

        self.SA_layers = nn.ModuleList()
        self.SA_layer_names = []
        self.downsample_times_map = {}
        c_in = 0
        for src_name in model_cfg['FEATURES_SOURCE']:
            if src_name in ['bev', 'raw_points']:
                continue
            self.downsample_times_map[src_name] = SA_cfg[src_name]['DOWNSAMPLE_FACTOR']
            if SA_cfg[src_name].get('INPUT_CHANNELS', None) is None:
                first = SA_cfg[src_name]['MLPS'][0]
                input_channels = first[0] if isinstance(first, (list, tuple)) else first
            else:
                input_channels = SA_cfg[src_name]['INPUT_CHANNELS']
            cur_layer, cur_num_c_out = self.build_local_aggregation_module(
                input_channels=input_channels, config=SA_cfg[src_name])
            self.SA_layers.append(cur_layer)
            self.SA_layer_names.append(src_name)
            c_in += cur_num_c_out
        if 'bev' in model_cfg['FEATURES_SOURCE']:
            c_in += num_bev_features
        if 'raw_points' in model_cfg['FEATURES_SOURCE']:
            self.SA_rawpoints, cur_num_c_out = self.build_local_aggregation_module(
                input_channels=num_rawpoint_features - 3, config=SA_cfg['raw_points'])
            c_in += cur_num_c_out
        self.vsa_point_feature_fusion = nn.Sequential(
            nn.Linear(c_in, model_cfg['NUM_OUTPUT_FEATURES'], bias=False),
            nn.BatchNorm1d(model_cfg['NUM_OUTPUT_FEATURES']),
            nn.ReLU(),
        )
        self.num_point_features = model_cfg['NUM_OUTPUT_FEATURES']
        self.num_point_features_before_fusion = c_in

    def interpolate_from_bev_features(self, keypoints, bev_features, batch_size, bev_stride):
        """keypoints (N1 + N2 + ..., 4), bev_features (B, C, H, W) -> (N1 + N2 + ..., C)"""
        x_idxs = (keypoints[:, 1] - self.point_cloud_range[0]) / self.voxel_size[0]
        y_idxs = (keypoints[:, 2] - self.point_cloud_range[1]) / self.voxel_size[1]
        x_idxs = x_idxs / bev_stride
        y_idxs = y_idxs / bev_stride
        return bev_interpolate(keypoints, x_idxs, y_idxs, bev_features)

    def get_sampled_points(self, batch_dict, return_indices=False):
        """-> keypoints (B * NUM_KEYPOINTS, 4) [bs_idx, x, y, z]"""
        batch_size = batch_dict['batch_size']
        if self.model_cfg['POINT_SOURCE'] == 'raw_points':
            src_points = batch_dict['points'][:, 1:4]
            batch_indices = batch_dict['points'][:, 0].long()
        else:
            src_points = get_voxel_centers(batch_dict['voxel_coords'][:, 1:4], downsample_times=1, voxel_size=self.voxel_size,
                                           point_cloud_range=self.point_cloud_range)
            batch_indices = batch_dict['voxel_coords'][:, 0].long()
        K = self.model_cfg['NUM_KEYPOINTS']
        rows = sample_keypoints(src_points, batch_indices, batch_size, K)                        # (B, K)
        batch_idx = torch.arange(batch_size, device=rows.device).view(-1, 1).repeat(1, K).view(-1, 1)
        keypoints = torch.cat((batch_idx.float(), src_points[rows.view(-1)].float()), dim=1)
        return (keypoints, rows) if return_indices else keypoints

    def keypoints_and_counts(self, batch_dict):
        """-> keypoints (M1 + M2 + ..., 4) and their int32 counts per scene: here NUM_KEYPOINTS of every scene."""
        keypoints = self.get_sampled_points(batch_dict)
        return keypoints, torch.full((batch_dict['batch_size'],), self.model_cfg['NUM_KEYPOINTS'], dtype=torch.int32,
                                     device=keypoints.device)

    def source_rows(self, src_name, xyz, xyz_features, xyz_bs_idxs, batch_dict):
        """The rows of one feature source that reach its layer: here all of them."""
        return xyz, xyz_features, xyz_bs_idxs

    @staticmethod
    def aggregate_keypoint_features_from_one_source(batch_size, aggregate_func, xyz, xyz_features, xyz_bs_idxs, new_xyz,
                                                    new_xyz_batch_cnt):
        xyz_batch_cnt = scene_counts(xyz_bs_idxs, batch_size)
        _, pooled_features = aggregate_func(xyz=xyz.contiguous(), xyz_batch_cnt=xyz_batch_cnt, new_xyz=new_xyz,
                                            new_xyz_batch_cnt=new_xyz_batch_cnt, features=xyz_features.contiguous())
        return pooled_features

    def forward(self, batch_dict):
        """batch_size, points (N, 1 + 3 + C) and / or voxel_coords, multi_scale_3d_features, spatial_features and its stride
        -> point_features_before_fusion, point_features (B * K, C), point_coords (B * K, 4)."""
        keypoints, new_xyz_batch_cnt = self.keypoints_and_counts(batch_dict)
        batch_size = batch_dict['batch_size']
        point_features_list = []
        if 'bev' in self.model_cfg['FEATURES_SOURCE']:
            point_features_list.append(self.interpolate_from_bev_features(
                keypoints, batch_dict['spatial_features'], batch_size, bev_stride=batch_dict['spatial_features_stride']))

        new_xyz = keypoints[:, 1:4].contiguous()

        if 'raw_points' in self.model_cfg['FEATURES_SOURCE']:
            raw_points = batch_dict['points']
            if raw_points.shape[1] <= 4:
                raise ValueError("FEATURES_SOURCE raw_points needs point features next to the coordinates")
            xyz, xyz_features, xyz_bs_idxs = self.source_rows('raw_points', raw_points[:, 1:4], raw_points[:, 4:], raw_points[:, 0],
                                                              batch_dict)
            point_features_list.append(self.aggregate_keypoint_features_from_one_source(
                batch_size=batch_size, aggregate_func=self.SA_rawpoints, xyz=xyz, xyz_features=xyz_features,
                xyz_bs_idxs=xyz_bs_idxs, new_xyz=new_xyz, new_xyz_batch_cnt=new_xyz_batch_cnt))

        for k, src_name in enumerate(self.SA_layer_names):
            cur = batch_dict['multi_scale_3d_features'][src_name]
            cur_coords = cur.indices
            xyz = get_voxel_centers(cur_coords[:, 1:4], downsample_times=self.downsample_times_map[src_name],
                                    voxel_size=self.voxel_size, point_cloud_range=self.point_cloud_range)
            xyz, xyz_features, xyz_bs_idxs = self.source_rows(src_name, xyz, cur.features, cur_coords[:, 0], batch_dict)
            point_features_list.append(self.aggregate_keypoint_features_from_one_source(
                batch_size=batch_size, aggregate_func=self.SA_layers[k], xyz=xyz, xyz_features=xyz_features,
                xyz_bs_idxs=xyz_bs_idxs, new_xyz=new_xyz, new_xyz_batch_cnt=new_xyz_batch_cnt))

        point_features = torch.cat(point_features_list, dim=-1)
        batch_dict['point_features_before_fusion'] = point_features.view(-1, point_features.shape[-1])
        point_features = self.vsa_point_feature_fusion(point_features.view(-1, point_features.shape[-1]))
        batch_dict['point_features'] = point_features
        batch_dict['point_coords'] = keypoints
        return batch_dict
