"""UNetV2 (pcdet/models/backbones_3d/spconv_unet.py), the backbone of Part-A2, over spconv_utils: SparseInverseConv3d, the
file's own SparseBasicBlock (convolutions without bias, unlike spconv_backbone's) and UNetV2 with the reference's attribute
names, indice_keys, BatchNorm settings, RETURN_ENCODED_TENSOR and last_pad, so that a reference checkpoint (spconv 2.x layout)
loads with strict=True.

The inverse convolution has no kernel of its own.  If the strided convolution that owns `indice_key`
computes out[o] = sum_t W[:, t, :] . in[nbr_out[o][t]], the inverse computes y[i] = sum_t W'[:, t, :] . x[nbr_in[i][t]]: the
same (input row, output row) pairs under the same tap index, no flip, with input and output exchanged -- spconv's rule.  Its
forward, data gradient and weight gradient are pda_spconv_gemm / pda_spconv_wgrad with the two index tables and the two row
counts of the rulebook exchanged.  The result lives on the input sites of that strided convolution, row for row
(Rulebook.in_indices), so the decoder's features line up with the encoder's and point_features with the input voxels.

Host reads of a UNetV2 forward: the four strided rulebook builds (spconv2, spconv3, spconv4, spconv_down2), nothing else.
Compact tensors only: a padded tensor (num_active) is refused, as every second stage refuses a padded batch."""
from functools import partial

import torch
import torch.nn as nn

from . import spconv_utils as spconv
from .pointnet2_batch_cuda import F32, _call, _chk
from .spconv_backbone import post_act_block as _encoder_block
from .spconv_utils import _plane, replace_feature
from .stage_common import workspace
from .voxel_utils import get_voxel_centers


class _InverseConvFunction(torch.autograd.Function):
    """The rulebook of the strided convolution read the other way round: rows are its input sites, sources its output sites."""

    @staticmethod
    def forward(ctx, features, weight, bias, book):
        cout, cin = weight.shape[0], weight.shape[-1]
        out = torch.empty((book.n_in, cout), dtype=F32, device=features.device)
        if book.n_in:
            _call("pda_spconv_gemm", features, features.data_ptr(), book.nbr_in.data_ptr(), _plane(weight, False).data_ptr(),
                  None if bias is None else bias.data_ptr(), out.data_ptr(), book.n_in, book.n_out, book.taps, cin, cout, 0, 0)
        ctx.save_for_backward(features, weight)
        ctx.book, ctx.has_bias = book, bias is not None
        return out

    @staticmethod
    def backward(ctx, grad):
        features, weight = ctx.saved_tensors
        book = ctx.book
        cout, cin = weight.shape[0], weight.shape[-1]
        grad = grad.contiguous()
        g_feat = g_w = g_b = None
        if ctx.needs_input_grad[0]:
            g_feat = torch.empty_like(features)
            if book.n_out:
                _call("pda_spconv_gemm", grad, grad.data_ptr(), book.nbr_out.data_ptr(), _plane(weight, True).data_ptr(), None,
                      g_feat.data_ptr(), book.n_out, book.n_in, book.taps, cin, cout, 1, 0)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            g_w = torch.empty_like(weight)
            g_b = torch.empty((cout,), dtype=F32, device=grad.device) if ctx.has_bias else None
            ws = workspace("pda_spconv_wgrad_workspace_bytes", (book.n_in, book.taps, cin, cout), "bad weight-gradient sizes",
                           grad.device)
            _call("pda_spconv_wgrad", grad, features.data_ptr(), grad.data_ptr(), book.nbr_in.data_ptr(), book.n_in, book.n_out,
                  book.taps, cin, cout, g_w.data_ptr(), None if g_b is None else g_b.data_ptr(), ws.data_ptr())
        return g_feat, g_w, g_b, None


def sparse_inverse_conv(features, weight, bias, book):
    """features (book.n_out, C_in) float32 on the output sites of the strided rulebook `book`, weight (C_out, kD, kH, kW, C_in),
    bias (C_out) or None -> (book.n_in, C_out) on its input sites.  Differentiable in all three."""
    if book.kind != 'spconv' or book.nbr_in is None:
        raise ValueError("an inverse convolution takes the rulebook of a strided convolution, got a %r one" % (book.kind,))
    if features.dim() != 2 or weight.dim() != 5 or features.shape[1] != weight.shape[-1] or features.shape[0] != book.n_out \
            or tuple(weight.shape[1:4]) != tuple(book.kernel_size):
        raise ValueError("features %s / weight %s do not fit the rulebook read backwards (%d rows, kernel %s)"
                         % (tuple(features.shape), tuple(weight.shape), book.n_out, book.kernel_size))
    if book.count_out is not None:
        raise NotImplementedError("the inverse convolution takes a compact rulebook, not a padded one")
    spconv._check_channels(weight.shape[-1], weight.shape[0])
    _chk(features, "features", F32)
    _chk(weight, "weight", F32)
    if bias is not None:
        _chk(bias, "bias", F32)
    return _InverseConvFunction.apply(features, weight, bias, book)


class SparseInverseConv3d(spconv.SparseConvolution):
    """spconv's SparseInverseConv3d: back from the output sites of the strided convolution that built `indice_key` to its
    input sites.  Stride and padding are that convolution's; the layer holds a weight of its own."""

    def __init__(self, in_channels, out_channels, kernel_size, indice_key, bias=True):
        if indice_key is None:
            raise ValueError("SparseInverseConv3d needs the indice_key of the strided convolution it inverts")
        super().__init__(in_channels, out_channels, kernel_size, bias=bias, subm=False, indice_key=indice_key)

    def extra_repr(self):
        return "%d, %d, kernel_size=%s, inverse of indice_key=%r" % (self.in_channels, self.out_channels, self.kernel_size,
                                                                     self.indice_key)

    def forward(self, input):
        if not isinstance(input, spconv.SparseConvTensor):
            raise TypeError("a sparse convolution takes a SparseConvTensor")
        if input.num_active is not None:
            raise NotImplementedError("SparseInverseConv3d takes a compact tensor, not a padded one (num_active)")
        book = input.indice_dict.get(self.indice_key)
        if book is None:
            raise ValueError("SparseInverseConv3d: no rulebook under indice_key %r -- the strided convolution of that key "
                             "runs first, on a tensor that shares this one's indice_dict" % (self.indice_key,))
        if book.kind != 'spconv':
            raise ValueError("SparseInverseConv3d: indice_key %r names the rulebook of a submanifold convolution" % (self.indice_key,))
        if input.features.shape[0] != book.n_out or list(input.spatial_shape) != list(book.out_shape):
            raise ValueError("SparseInverseConv3d: %d rows on grid %s, the convolution of indice_key %r left %d on %s"
                             % (input.features.shape[0], input.spatial_shape, self.indice_key, book.n_out, book.out_shape))
        if book.in_indices is None:
            raise ValueError("SparseInverseConv3d: the rulebook under %r does not keep its input sites (a SparseConv3d layer "
                             "sets Rulebook.in_indices)" % (self.indice_key,))
        features = sparse_inverse_conv(input.features.contiguous(), self.weight, self.bias, book)
        return spconv.SparseConvTensor(features, book.in_indices, book.in_shape, input.batch_size, input.indice_dict)


def post_act_block(in_channels, out_channels, kernel_size, indice_key=None, stride=1, padding=0, conv_type='subm', norm_fn=None):
    """spconv_backbone.post_act_block with the 'inverseconv' kind built here."""
    if conv_type == 'inverseconv':
        conv = SparseInverseConv3d(in_channels, out_channels, kernel_size, indice_key=indice_key, bias=False)
        return spconv.SparseSequential(conv, norm_fn(out_channels), nn.ReLU())
    return _encoder_block(in_channels, out_channels, kernel_size, indice_key=indice_key, stride=stride, padding=padding,
                          conv_type=conv_type, norm_fn=norm_fn)


class SparseBasicBlock(spconv.SparseModule):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, indice_key=None, norm_fn=None):
        super().__init__()
        self.conv1 = spconv.SubMConv3d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=False, indice_key=indice_key)
        self.bn1 = norm_fn(planes)
        self.relu = nn.ReLU()
        self.conv2 = spconv.SubMConv3d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False, indice_key=indice_key)
        self.bn2 = norm_fn(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x.features
        out = self.conv1(x)
        out = replace_feature(out, self.bn1(out.features))
        out = replace_feature(out, self.relu(out.features))
        out = self.conv2(out)
        out = replace_feature(out, self.bn2(out.features))
        if self.downsample is not None:
            identity = self.downsample(x)
        out = replace_feature(out, out.features + identity)
        out = replace_feature(out, self.relu(out.features))
        return out


class UNetV2(nn.Module):
    """Sparse-convolution UNet for point-wise features (Shi et al., "From Points to Parts", arXiv 1907.03670)."""

    def __init__(self, model_cfg, input_channels, grid_size, voxel_size, point_cloud_range, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        grid = [int(v) for v in grid_size]
        self.sparse_shape = [grid[2] + 1, grid[1], grid[0]]
        self.voxel_size = voxel_size
        self.point_cloud_range = point_cloud_range

        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        self.conv_input = spconv.SparseSequential(
            spconv.SubMConv3d(input_channels, 16, 3, padding=1, bias=False, indice_key='subm1'), norm_fn(16), nn.ReLU())
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

        if self.model_cfg.get('RETURN_ENCODED_TENSOR', True):
            last_pad = self.model_cfg.get('last_pad', 0)
            self.conv_out = spconv.SparseSequential(
                spconv.SparseConv3d(64, 128, (3, 1, 1), stride=(2, 1, 1), padding=last_pad, bias=False,
                                    indice_key='spconv_down2'), norm_fn(128), nn.ReLU())
        else:
            self.conv_out = None

        # decoder: level 4 -> 3 -> 2 -> 1
        self.conv_up_t4 = SparseBasicBlock(64, 64, indice_key='subm4', norm_fn=norm_fn)
        self.conv_up_m4 = block(128, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm4')
        self.inv_conv4 = block(64, 64, 3, norm_fn=norm_fn, indice_key='spconv4', conv_type='inverseconv')

        self.conv_up_t3 = SparseBasicBlock(64, 64, indice_key='subm3', norm_fn=norm_fn)
        self.conv_up_m3 = block(128, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm3')
        self.inv_conv3 = block(64, 32, 3, norm_fn=norm_fn, indice_key='spconv3', conv_type='inverseconv')

        self.conv_up_t2 = SparseBasicBlock(32, 32, indice_key='subm2', norm_fn=norm_fn)
        self.conv_up_m2 = block(64, 32, 3, norm_fn=norm_fn, indice_key='subm2')
        self.inv_conv2 = block(32, 16, 3, norm_fn=norm_fn, indice_key='spconv2', conv_type='inverseconv')

        self.conv_up_t1 = SparseBasicBlock(16, 16, indice_key='subm1', norm_fn=norm_fn)
        self.conv_up_m1 = block(32, 16, 3, norm_fn=norm_fn, indice_key='subm1')

        self.conv5 = spconv.SparseSequential(block(16, 16, 3, norm_fn=norm_fn, padding=1, indice_key='subm1'))
        self.num_point_features = 16

    def UR_block_forward(self, x_lateral, x_bottom, conv_t, conv_m, conv_inv):
        x_trans = conv_t(x_lateral)
        x = x_trans
        x = replace_feature(x, torch.cat((x_bottom.features, x_trans.features), dim=1))
        x_m = conv_m(x)
        x = self.channel_reduction(x, x_m.features.shape[1])
        x = replace_feature(x, x_m.features + x.features)
        x = conv_inv(x)
        return x

    @staticmethod
    def channel_reduction(x, out_channels):
        """x.features (N, C1) -> (N, C2), C2 dividing C1: the sum over each run of C1 / C2 channels."""
        features = x.features
        n, in_channels = features.shape
        assert (in_channels % out_channels == 0) and (in_channels >= out_channels)
        x = replace_feature(x, features.view(n, out_channels, -1).sum(dim=2))
        return x

    def forward(self, batch_dict):
        """batch_dict: batch_size, voxel_features (num_voxels, C), voxel_coords (num_voxels, 4) [batch_idx, z, y, x] ->
        encoded_spconv_tensor (+ _stride 8) unless RETURN_ENCODED_TENSOR is off, point_features (num_voxels, 16) row-aligned
        with the input voxels, point_coords (num_voxels, 4) [batch_idx, x, y, z] of the voxel centres."""
        if batch_dict.get('voxel_num_active') is not None:
            raise NotImplementedError("UNetV2 takes a compact batch, not a padded one (voxel_num_active)")
        voxel_features, voxel_coords = batch_dict['voxel_features'], batch_dict['voxel_coords']
        x = spconv.SparseConvTensor(features=voxel_features, indices=voxel_coords.int(), spatial_shape=self.sparse_shape,
                                    batch_size=batch_dict['batch_size'])
        x = self.conv_input(x)
        x_conv1 = self.conv1(x)
        x_conv2 = self.conv2(x_conv1)
        x_conv3 = self.conv3(x_conv2)
        x_conv4 = self.conv4(x_conv3)

        if self.conv_out is not None:
            out = self.conv_out(x_conv4)
            batch_dict['encoded_spconv_tensor'] = out
            batch_dict['encoded_spconv_tensor_stride'] = 8

        x_up4 = self.UR_block_forward(x_conv4, x_conv4, self.conv_up_t4, self.conv_up_m4, self.inv_conv4)
        x_up3 = self.UR_block_forward(x_conv3, x_up4, self.conv_up_t3, self.conv_up_m3, self.inv_conv3)
        x_up2 = self.UR_block_forward(x_conv2, x_up3, self.conv_up_t2, self.conv_up_m2, self.inv_conv2)
        x_up1 = self.UR_block_forward(x_conv1, x_up2, self.conv_up_t1, self.conv_up_m1, self.conv5)

        batch_dict['point_features'] = x_up1.features
        point_coords = get_voxel_centers(x_up1.indices[:, 1:], downsample_times=1, voxel_size=self.voxel_size,
                                         point_cloud_range=self.point_cloud_range)
        batch_dict['point_coords'] = torch.cat((x_up1.indices[:, 0:1].float(), point_coords), dim=1)
        return batch_dict
