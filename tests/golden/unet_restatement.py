"""UNetV2 restated densely on the CPU, on top of sparse_conv_restatement.py.  The inverse convolution
of a strided convolution (kernel k, stride s, padding p, input grid `in_shape`) is torch.nn.functional.conv_transpose3d with
the layer's weight W' (C_out, kD, kH, kW, C_in) permuted to (C_in, C_out, kD, kH, kW), the same stride and padding, and the
output_padding that makes the result `in_shape` large -- y[i] = sum over (o, t) with s * o - p + t = i of W'[:, t, :] . x[o], no
flip --, masked to the strided convolution's input sites.  BatchNorm1d and ReLU act on the active rows.  dense_unet() walks a
UNetV2 by class names and attributes only; none of this uses the code under test."""
import numpy as np
import torch
import torch.nn.functional as F

import sparse_conv_restatement as rs


def output_padding(in_shape, out_shape, k, s, p):
    op = tuple(int(i) - ((int(o) - 1) * ss - 2 * pp + kk) for i, o, kk, ss, pp in zip(in_shape, out_shape, k, s, p))
    assert all(0 <= v < ss for v, ss in zip(op, s)), (op, s)
    return op


def inverse_dense(values, weight, bias, k, s, p, in_shape):
    """values (B, C_in, D', H', W') on the strided convolution's output grid -> (B, C_out, D, H, W) on its input grid."""
    k, s, p = rs.triple(k), rs.triple(s), rs.triple(p)
    op = output_padding(in_shape, values.shape[2:], k, s, p)
    out = F.conv_transpose3d(values, weight.permute(4, 0, 1, 2, 3), bias, stride=s, padding=p, output_padding=op)
    assert list(out.shape[2:]) == [int(v) for v in in_shape]
    return out


def inverse_conv_rows(features, out_sites, in_sites, in_shape, batch, weight, bias, k, s, p):
    """features (M, C_in) on `out_sites` (M, 4), the output sites of the strided convolution of `in_sites` (N, 4) -> the inverse
    convolution's rows (N, C_out) in the order of in_sites."""
    k, s, p = rs.triple(k), rs.triple(s), rs.triple(p)
    oshape = rs.out_shape(in_shape, k, s, p)
    dense = inverse_dense(rs.scatter_dense(features, out_sites, oshape, batch), weight, bias, k, s, p, in_shape)
    st = torch.as_tensor(np.asarray(in_sites, np.int64))
    return dense.permute(0, 2, 3, 4, 1)[st[:, 0], st[:, 1], st[:, 2], st[:, 3]]


def dense_run(module, x, books):
    """sparse_conv_restatement.dense_run plus SparseInverseConv3d.  books: indice_key -> (input mask, stride, padding) of the
    strided convolutions met so far."""
    name = type(module).__name__
    if name == 'SparseSequential':
        for child in module._modules.values():
            x = dense_run(child, x, books)
        return x
    if name == 'SparseConv3d':
        books[module.indice_key] = (x.mask, module.stride, module.padding)
    if name == 'SparseInverseConv3d':
        mask, s, p = books[module.indice_key]
        v = inverse_dense(x.values, module.weight, module.bias, module.kernel_size, s, p, mask.shape[1:])
        return rs.DenseSparse(v * mask.unsqueeze(1).to(v.dtype), mask)
    return rs.dense_run(module, x)


def ur_block(x_lateral, x_bottom, conv_t, conv_m, conv_inv, books):
    x_trans = dense_run(conv_t, x_lateral, books)
    x = x_trans.with_rows(torch.cat((x_bottom.rows(), x_trans.rows()), dim=1))
    x_m = dense_run(conv_m, x, books).rows()
    rows = x.rows()
    reduced = rows.view(rows.shape[0], x_m.shape[1], -1).sum(dim=2)
    return dense_run(conv_inv, x.with_rows(x_m + reduced), books)


def dense_unet(model, features, indices, batch):
    """UNetV2 densely: {'out': DenseSparse (when the model has conv_out), 'up1': DenseSparse, 'point_features': (N, 16) rows in
    the order of `indices`}."""
    books = {}
    x = dense_run(model.conv_input, rs.dense_input(features, indices, model.sparse_shape, batch), books)
    c1 = dense_run(model.conv1, x, books)
    c2 = dense_run(model.conv2, c1, books)
    c3 = dense_run(model.conv3, c2, books)
    c4 = dense_run(model.conv4, c3, books)
    res = {}
    if model.conv_out is not None:
        res['out'] = dense_run(model.conv_out, c4, books)
    up4 = ur_block(c4, c4, model.conv_up_t4, model.conv_up_m4, model.inv_conv4, books)
    up3 = ur_block(c3, up4, model.conv_up_t3, model.conv_up_m3, model.inv_conv3, books)
    up2 = ur_block(c2, up3, model.conv_up_t2, model.conv_up_m2, model.inv_conv2, books)
    up1 = ur_block(c1, up2, model.conv_up_t1, model.conv_up_m1, model.conv5, books)
    res['up1'] = up1
    st = torch.as_tensor(np.asarray(indices, np.int64))
    res['point_features'] = up1.values.permute(0, 2, 3, 4, 1)[st[:, 0], st[:, 1], st[:, 2], st[:, 3]]
    return res
