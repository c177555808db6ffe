"""VoxelBackBone8x and VoxelResBackBone8x (pcdet/models/backbones_3d/spconv_backbone.py) over spconv_utils: the same
constructor signatures, sparse_shape (grid_size reversed, + 1 in z), `last_pad` key, batch_dict outputs
(encoded_spconv_tensor, encoded_spconv_tensor_stride, multi_scale_3d_features, multi_scale_3d_strides), num_point_features
and backbone_channels, and the same module names, so a reference checkpoint (spconv 2.x layout) loads with strict=True.
BatchNorm1d(eps=1e-3, momentum=0.01) stays a plain module over the active rows.  A forward builds one rulebook
per indice_key -- subm1, spconv2, subm2, spconv3, subm3, spconv4, subm4, spconv_down2; the Res form res1..res4 in place of
subm2..subm4 and next to subm1 -- and makes four host reads, one per strided convolution.  A padded batch
(voxel_num_active) makes none: the rulebooks keep their counts on the device, the BatchNorm1d modules run
through the counted kernels, the tail of a SparseBasicBlock -- relu(bn2(x) + identity) -- is one counted kernel pair
(spconv_utils.counted_batch_norm_add_relu; PDA_RES_BN=composed keeps BatchNorm, `+` and ReLU apart, with the same bits), and
model_cfg PADDED_CAPS says how many rows each strided convolution reserves."""
from functools import partial

import torch.nn as nn

from . import spconv_utils as spconv
from .config import fused_or_composed
from .spconv_utils import counted_batch_norm, counted_batch_norm_add_relu, replace_feature


def post_act_block(in_channels, out_channels, kernel_size, indice_key=None, stride=1, padding=0, conv_type='subm', norm_fn=None):
    if conv_type == 'subm':
        conv = spconv.SubMConv3d(in_channels, out_channels, kernel_size, bias=False, indice_key=indice_key)
    elif conv_type == 'spconv':
        conv = spconv.SparseConv3d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=False,
                                   indice_key=indice_key)
    elif conv_type == 'inverseconv':
        conv = spconv.SparseInverseConv3d(in_channels, out_channels, kernel_size, indice_key=indice_key, bias=False)
    else:
        raise NotImplementedError
    return spconv.SparseSequential(conv, norm_fn(out_channels), nn.ReLU())


class SparseBasicBlock(spconv.SparseModule):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, norm_fn=None, downsample=None, indice_key=None):
        super().__init__()
        assert norm_fn is not None
        bias = norm_fn is not None
        self.conv1 = spconv.SubMConv3d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=bias, indice_key=indice_key)
        self.bn1 = norm_fn(planes)
        self.relu = nn.ReLU()
        self.conv2 = spconv.SubMConv3d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=bias, indice_key=indice_key)
        self.bn2 = norm_fn(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x
        out = self.conv1(x)
        if x.num_active is not None:          # padded: counted BatchNorm, bn1's ReLU folded in; dead rows stay exact zeros
            out = replace_feature(out, counted_batch_norm(self.bn1, out.features, out.num_active, out.status, relu=True))
            out = self.conv2(out)
            # PDA_RES_BN=composed: bn2, `+` and ReLU as three steps; the fused tail gives the same bits in one pass
            if fused_or_composed("PDA_RES_BN") == "fused" and self.downsample is None:
                return replace_feature(out, counted_batch_norm_add_relu(self.bn2, out.features, identity.features.contiguous(),
                                                                        out.num_active, out.status))
            out = replace_feature(out, counted_batch_norm(self.bn2, out.features, out.num_active, out.status, relu=False))
        else:
            out = replace_feature(out, self.bn1(out.features))
            out = replace_feature(out, self.relu(out.features))
            out = self.conv2(out)
            out = replace_feature(out, self.bn2(out.features))
        if self.downsample is not None:
            identity = self.downsample(x)
        out = replace_feature(out, out.features + identity.features)
        out = replace_feature(out, self.relu(out.features))
        return out


class _VoxelBackBone(nn.Module):
    """What the two backbones share: the input layer, the output layer and the forward."""
    LEVEL4 = 64          # channels of conv4

    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        grid = [int(v) for v in grid_size]
        self.sparse_shape = [grid[2] + 1, grid[1], grid[0]]
        self.conv_input = spconv.SparseSequential(
            spconv.SubMConv3d(input_channels, 16, 3, padding=1, bias=False, indice_key='subm1'), norm_fn(16), nn.ReLU())
        self.build_levels(norm_fn)
        last_pad = model_cfg.get('last_pad', 0)
        self.conv_out = spconv.SparseSequential(
            spconv.SparseConv3d(self.LEVEL4, 128, (3, 1, 1), stride=(2, 1, 1), padding=last_pad, bias=False,
                                indice_key='spconv_down2'), norm_fn(128), nn.ReLU())
        self.num_point_features = 128
        self.backbone_channels = {'x_conv1': 16, 'x_conv2': 32, 'x_conv3': 64, 'x_conv4': self.LEVEL4}

    def forward(self, batch_dict):
        """batch_dict: batch_size, voxel_features (num_voxels, C), voxel_coords (num_voxels, 4) [batch_idx, z, y, x].
        With voxel_num_active (a device int32; voxel_utils.collate_voxels_padded) the rows are a capacity and the whole
        forward reads nothing back: the strided convolutions reserve model_cfg PADDED_CAPS[indice_key] rows (default: the
        bound that cannot overflow), and voxel_status collects the flags (spconv_utils.padded_report)."""
        voxel_features, voxel_coords = batch_dict['voxel_features'], batch_dict['voxel_coords']
        num_active = batch_dict.get('voxel_num_active')
        x = spconv.SparseConvTensor(features=voxel_features, indices=voxel_coords.int(), spatial_shape=self.sparse_shape,
                                    batch_size=batch_dict['batch_size'], num_active=num_active,
                                    status=None if num_active is None else batch_dict.get('voxel_status'))
        if num_active is not None:
            x.caps = {key: int(rows) for key, rows in (self.model_cfg.get('PADDED_CAPS') or {}).items()}
            batch_dict['voxel_status'] = x.status
        x = self.conv_input(x)
        x_conv1 = self.conv1(x)
        x_conv2 = self.conv2(x_conv1)
        x_conv3 = self.conv3(x_conv2)
        x_conv4 = self.conv4(x_conv3)
        out = self.conv_out(x_conv4)
        batch_dict.update({'encoded_spconv_tensor': out, 'encoded_spconv_tensor_stride': 8})
        batch_dict.update({'multi_scale_3d_features': {'x_conv1': x_conv1, 'x_conv2': x_conv2, 'x_conv3': x_conv3,
                                                       'x_conv4': x_conv4}})
        batch_dict.update({'multi_scale_3d_strides': {'x_conv1': 1, 'x_conv2': 2, 'x_conv3': 4, 'x_conv4': 8}})
        return batch_dict


class VoxelBackBone8x(_VoxelBackBone):
    def build_levels(self, norm_fn):
        block = post_act_block
        self.conv1 = spconv.SparseSequential(block(16, 16, 3, norm_fn=norm_fn, padding=1, indice_key='subm1'))
        self.conv2 = spconv.SparseSequential(
            block(16, 32, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv2', conv_type='spconv'),
            block(32, 32, 3, norm_fn=norm_fn, padding=1, indice_key='subm2'),
            block(32, 32, 3, norm_fn=norm_fn, padding=1, indice_key='subm2'))
        self.conv3 = spconv.SparseSequential(
            block(32, 64, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv3', conv_type='spconv'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm3'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm3'))
        self.conv4 = spconv.SparseSequential(
            block(64, 64, 3, norm_fn=norm_fn, stride=2, padding=(0, 1, 1), indice_key='spconv4', conv_type='spconv'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm4'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm4'))


class VoxelResBackBone8x(_VoxelBackBone):
    LEVEL4 = 128

    def build_levels(self, norm_fn):
        block = post_act_block
        self.conv1 = spconv.SparseSequential(
            SparseBasicBlock(16, 16, norm_fn=norm_fn, indice_key='res1'),
            SparseBasicBlock(16, 16, norm_fn=norm_fn, indice_key='res1'))
        self.conv2 = spconv.SparseSequential(
            block(16, 32, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv2', conv_type='spconv'),
            SparseBasicBlock(32, 32, norm_fn=norm_fn, indice_key='res2'),
            SparseBasicBlock(32, 32, norm_fn=norm_fn, indice_key='res2'))
        self.conv3 = spconv.SparseSequential(
            block(32, 64, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv3', conv_type='spconv'),
            SparseBasicBlock(64, 64, norm_fn=norm_fn, indice_key='res3'),
            SparseBasicBlock(64, 64, norm_fn=norm_fn, indice_key='res3'))
        self.conv4 = spconv.SparseSequential(
            block(64, 128, 3, norm_fn=norm_fn, stride=2, padding=(0, 1, 1), indice_key='spconv4', conv_type='spconv'),
            SparseBasicBlock(128, 128, norm_fn=norm_fn, indice_key='res4'),
            SparseBasicBlock(128, 128, norm_fn=norm_fn, indice_key='res4'))
