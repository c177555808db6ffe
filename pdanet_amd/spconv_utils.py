"""Sparse 3D convolution on the device under the names the reference uses (pcdet/utils/spconv_utils.py and the part of
spconv 2.x that pcdet's voxel backbones touch): SparseConvTensor, SparseModule, SparseSequential, SubMConv3d, SparseConv3d,
replace_feature and find_all_spconv_keys (SparseConvTranspose3d exists to refuse, and so does SparseInverseConv3d under this
name: the inverse convolution is spconv_unet.SparseInverseConv3d).  spconv itself is not a dependency; the contract is DESIGN.md section 7.

A convolution is two stages.  The index stage (csrc/sparse_conv_index.hip) reads coordinates only and leaves a Rulebook: the
output sites and, per (row, tap), the row read (nbr_out) and, for a strided convolution, the row written (nbr_in).  A
rulebook is built once per `indice_key` and kept in the tensor's indice_dict, so every convolution that names the key
reuses it.  The feature stage (csrc/sparse_conv.hip) is a gather-GEMM over the rulebook: forward, data gradient and weight
gradient, float32 on the exact f32-input MFMA, without float atomics.

Output rows of a strided convolution come in ascending linear key ((b * D' + z) * H' + y) * W' + x -- spconv's own order
depends on hash insertion; everything downstream (dense(), BatchNorm over rows, voxel queries through a dense index map)
is order-free.  Weights keep spconv 2.x's layout (C_out, kD, kH, kW, C_in), the shapes a reference checkpoint holds.

Host reads: a strided build reads the output count and the flag word in one copy (BatchNorm must see exactly the live rows);
that read is where duplicate coordinates, coordinates outside the grid and overflow raise.  A submanifold build reads
nothing unless check=True.  With a rulebook in place forward and backward read nothing back and allocate through torch
only, so they are graph-capturable.

The padded form reads nothing at all: a SparseConvTensor that carries `num_active` (a device int32)
holds `cap` rows of which the first *num_active are live; the dead rows have indices -1, rulebook rows -1 and, after every
counted BatchNorm, features exactly 0.  The index stage takes its input count from the device and leaves the output count
there (Rulebook.count_out), BatchNorm runs through pda_bn_relu_*_counted, and what would have raised -- duplicate or outside
coordinates, more output sites than the capacity, a BatchNorm over fewer than two rows -- is ORed into the tensor's `status`
word instead, which padded_report reads whenever the caller likes."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import param_cache
from .pointpillar_scatter import pillar_scatter
from .pointnet2_batch_cuda import F32, I32, _buffers_written, _call, _chk, bn_relu_scratch_bytes
from .stage_common import workspace

FLAG_DUPLICATE, FLAG_OUTSIDE = 1, 2
FLAG_OVERFLOW, FLAG_FEW_ROWS = 4, 8          # the padded form only: what the compact form raises for
MAX_CHANNELS = 128
ROW_TILE = 64              # output rows of a workgroup of the gather-GEMM (csrc/sparse_conv.hip SC_ROWS)
_KEY_LIMIT = 2 ** 31


def _triple(v, name):
    if isinstance(v, (list, tuple)):
        if len(v) != 3:
            raise ValueError("%s must be an int or three ints, got %r" % (name, v))
        return tuple(int(x) for x in v)
    return (int(v),) * 3


def conv_output_shape(spatial_shape, kernel_size, stride, padding):
    """(in + 2p - k) // s + 1 per axis."""
    return [(int(i) + 2 * p - k) // s + 1 for i, k, s, p in zip(spatial_shape, kernel_size, stride, padding)]


def _check_key_range(batch_size, shape, what):
    cells = int(batch_size)
    for v in shape:
        cells *= int(v)
    if cells >= _KEY_LIMIT:
        raise ValueError("%s: batch %d x grid %s reaches 2^31 cells, the most an int32 key holds"
                         % (what, batch_size, list(shape)))


def _raise_on_flags(flags, what):
    if flags & FLAG_OUTSIDE:
        raise ValueError("%s: a coordinate lies outside [0, B) x [0, D) x [0, H) x [0, W)" % what)
    if flags & FLAG_DUPLICATE:
        raise ValueError("%s: two rows share a coordinate" % what)


class Rulebook:
    """What the index stage leaves for one (input sites, kernel, stride, padding): out_indices (n_out, 4), spatial shape of
    the output, nbr_out (n_out, T), nbr_in (n_in, T) or None for a submanifold convolution (nbr_out with mirrored taps).
    in_indices: the input sites (n_in, 4) of a strided book built by a layer -- what spconv_unet.SparseInverseConv3d returns to."""

    def __init__(self, kind, kernel_size, stride, padding, in_shape, out_shape, n_in, out_indices, nbr_out, nbr_in,
                 count_out=None):
        self.count_out = count_out          # padded form: device int32 (1), the live output rows; n_out is then the capacity
        self.in_indices = None
        self.kind, self.kernel_size, self.stride, self.padding = kind, kernel_size, stride, padding
        self.in_shape, self.out_shape, self.n_in = list(in_shape), list(out_shape), n_in
        self.out_indices, self.nbr_out, self.nbr_in = out_indices, nbr_out, nbr_in
        self.n_out = out_indices.shape[0]
        self.taps = kernel_size[0] * kernel_size[1] * kernel_size[2]

    def matches(self, kind, kernel_size, stride, padding, in_shape, n_in):
        return (self.kind, self.kernel_size, self.stride, self.padding, self.in_shape, self.n_in) == \
            (kind, kernel_size, stride, padding, list(in_shape), n_in)


def _indices_ok(indices):
    _chk(indices, "indices", I32)
    if indices.dim() != 2 or indices.shape[1] != 4:
        raise ValueError("indices must be (N, 4) int32 (b, z, y, x), got %s" % (tuple(indices.shape),))


def _count_ok(t, name):
    """A device word of the padded form: one int32."""
    if not isinstance(t, torch.Tensor) or t.dtype != I32 or t.numel() != 1:
        raise ValueError("%s must be an int32 tensor of one element, got %s"
                         % (name, "%s %s" % (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
    return t


def _counted_args(count, status):
    if status is None:
        raise ValueError("a count comes with a status word (one device int32 that the kernels OR their flags into)")
    _chk(_count_ok(count, "count"), "count", I32)
    _chk(_count_ok(status, "status"), "status", I32)


def build_subm_rulebook(indices, spatial_shape, batch_size, kernel_size, check=False, count=None, status=None):
    """The rulebook of a SubMConv3d (odd kernel, stride 1): no host read unless check=True, which reads the flag word and
    raises for duplicate or out-of-range coordinates.  count (with status): the padded form -- the rows from *count on are
    dead, flags go to *status, check is ignored and nothing is read."""
    _indices_ok(indices)
    k = _triple(kernel_size, "kernel_size")
    if any(v % 2 != 1 for v in k):
        raise NotImplementedError("SubMConv3d takes an odd kernel, got %s" % (k,))
    _check_key_range(batch_size, spatial_shape, "SubMConv3d")
    n, T = indices.shape[0], k[0] * k[1] * k[2]
    D, H, W = (int(v) for v in spatial_shape)
    nbr = torch.empty((n, T), dtype=I32, device=indices.device)
    book = Rulebook('subm', k, (1, 1, 1), tuple(v // 2 for v in k), spatial_shape, spatial_shape, n, indices, nbr, None,
                    count_out=count)
    if n == 0:
        return book
    if count is not None:
        _counted_args(count, status)
        ws = workspace("pda_spconv_index_workspace_bytes", (n, 0, 1), "%d rows are too many for the index stage" % n, indices.device)
        _call("pda_spconv_index_subm_counted", indices, indices.data_ptr(), n, count.data_ptr(), int(batch_size), D, H, W, k[0], k[1],
              k[2], nbr.data_ptr(), status.data_ptr(), ws.data_ptr())
        return book
    stat = torch.empty((2,), dtype=I32, device=indices.device)
    ws = workspace("pda_spconv_index_workspace_bytes", (n, 0, 1), "%d rows are too many for the index stage" % n, indices.device)
    _call("pda_spconv_index_subm", indices, indices.data_ptr(), n, int(batch_size), D, H, W, k[0], k[1], k[2], nbr.data_ptr(),
          stat.data_ptr(), ws.data_ptr())
    if check:
        _raise_on_flags(int(stat[1].item()), "SubMConv3d")
    return book


def build_strided_rulebook(indices, spatial_shape, batch_size, kernel_size, stride, padding, cap=None, count=None, status=None):
    """The rulebook of a SparseConv3d.  One host read: the output count and the flag word.  cap: the rows reserved for the
    output (default: an upper bound that cannot overflow); a count above it raises and nothing is written past it.
    count (with status): the padded form -- no host read; the output keeps all cap rows, Rulebook.count_out says how many are
    live, and an overflow keeps the cap smallest keys and sets FLAG_OVERFLOW in *status."""
    _indices_ok(indices)
    k, s, p = _triple(kernel_size, "kernel_size"), _triple(stride, "stride"), _triple(padding, "padding")
    D, H, W = (int(v) for v in spatial_shape)
    out_shape = conv_output_shape((D, H, W), k, s, p)
    if min(out_shape) < 1:
        raise ValueError("SparseConv3d: kernel %s does not fit the padded grid %s" % (k, [D, H, W]))
    _check_key_range(batch_size, spatial_shape, "SparseConv3d")
    _check_key_range(batch_size, out_shape, "SparseConv3d (output grid)")
    n, T = indices.shape[0], k[0] * k[1] * k[2]
    dev = indices.device
    cands = 1
    for a in range(3):
        cands *= -(-k[a] // s[a])
    if cap is None:
        cap = min(n * cands, int(batch_size) * out_shape[0] * out_shape[1] * out_shape[2])
    cap = int(cap)
    if n == 0:
        return Rulebook('spconv', k, s, p, spatial_shape, out_shape, 0, torch.empty((0, 4), dtype=I32, device=dev),
                        torch.empty((0, T), dtype=I32, device=dev), torch.empty((0, T), dtype=I32, device=dev))
    out_indices = torch.empty((cap, 4), dtype=I32, device=dev)
    nbr_out = torch.empty((cap, T), dtype=I32, device=dev)
    nbr_in = torch.empty((n, T), dtype=I32, device=dev)
    ws = workspace("pda_spconv_index_workspace_bytes", (n, cap, cands), "%d rows are too many for the index stage" % n, dev)
    if count is not None:
        _counted_args(count, status)
        count_out = torch.empty((1,), dtype=I32, device=dev)
        _call("pda_spconv_index_strided_counted", indices, indices.data_ptr(), n, count.data_ptr(), int(batch_size), D, H, W, k[0],
              k[1], k[2], s[0], s[1], s[2], p[0], p[1], p[2], cap, out_indices.data_ptr(), nbr_out.data_ptr(), nbr_in.data_ptr(),
              count_out.data_ptr(), status.data_ptr(), ws.data_ptr())
        return Rulebook('spconv', k, s, p, spatial_shape, out_shape, n, out_indices, nbr_out, nbr_in, count_out=count_out)
    stat = torch.empty((2,), dtype=I32, device=dev)
    _call("pda_spconv_index_strided", indices, indices.data_ptr(), n, int(batch_size), D, H, W, k[0], k[1], k[2], s[0], s[1], s[2],
          p[0], p[1], p[2], cap, out_indices.data_ptr(), nbr_out.data_ptr(), nbr_in.data_ptr(), stat.data_ptr(), ws.data_ptr())
    count, flags = stat.tolist()                                  # the one host read
    _raise_on_flags(flags, "SparseConv3d")
    if count > cap:
        raise ValueError("SparseConv3d: %d output sites, room for %d" % (count, cap))
    return Rulebook('spconv', k, s, p, spatial_shape, out_shape, n, out_indices[:count], nbr_out[:count], nbr_in)


# [plane of W, plane of W^T] per weight, found by storage address: the forward packs, the backward of the same iteration hits
_PLANES = param_cache.Store(under_capture=False, weights_only=True)


def _pad16(c):
    return (c + 15) // 16 * 16


def _pack(weight, transposed):
    """weight (C_out, kD, kH, kW, C_in) -> the per-tap planes of pda_spconv_gemm: (T, pad16(C_in), C_out), or transposed
    (T, C_out, pad16(C_in)); the padding is zero."""
    cout, cin = weight.shape[0], weight.shape[-1]
    w = weight.detach().reshape(cout, -1, cin)
    if transposed:
        return F.pad(w.permute(1, 0, 2), (0, _pad16(cin) - cin)).contiguous()
    return F.pad(w.permute(1, 2, 0), (0, 0, 0, _pad16(cin) - cin)).contiguous()


def _plane(weight, transposed):
    pair = _PLANES.get_at(weight, lambda: [None, None], extra=tuple(weight.shape)) if weight.is_contiguous() else None
    slot = 1 if transposed else 0
    if pair is None:                                              # capturing, or not a parameter: pack here and now
        return _pack(weight, transposed)
    if pair[slot] is None:
        pair[slot] = _pack(weight, transposed)
    return pair[slot]


def _check_channels(cin, cout):
    if not (1 <= cin <= MAX_CHANNELS and 16 <= cout <= MAX_CHANNELS and cout % 16 == 0):
        raise NotImplementedError("sparse convolution kernels take C_in in [1, %d] and C_out a multiple of 16 up to %d, got "
                                  "C_in=%d, C_out=%d" % (MAX_CHANNELS, MAX_CHANNELS, cin, cout))


class _SparseConvFunction(torch.autograd.Function):
    """Both kinds of convolution: the rulebook says which."""

    @staticmethod
    def forward(ctx, features, weight, bias, book):
        cout, cin = weight.shape[0], weight.shape[-1]
        out = torch.empty((book.n_out, cout), dtype=F32, device=features.device)
        if book.n_out:
            _call("pda_spconv_gemm", features, features.data_ptr(), book.nbr_out.data_ptr(), _plane(weight, False).data_ptr(),
                  None if bias is None else bias.data_ptr(), out.data_ptr(), book.n_out, book.n_in, book.taps, cin, cout, 0, 0)
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
            if book.n_in and book.n_out:
                subm = book.nbr_in is None
                nbr = book.nbr_out if subm else book.nbr_in
                _call("pda_spconv_gemm", grad, grad.data_ptr(), nbr.data_ptr(), _plane(weight, True).data_ptr(), None,
                      g_feat.data_ptr(), book.n_in, book.n_out, book.taps, cin, cout, 1, 1 if subm else 0)
            else:
                g_feat.zero_()
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            g_w = torch.empty_like(weight)
            g_b = torch.empty((cout,), dtype=F32, device=grad.device) if ctx.has_bias else None
            ws = workspace("pda_spconv_wgrad_workspace_bytes", (book.n_out, book.taps, cin, cout), "bad weight-gradient sizes",
                           grad.device)
            _call("pda_spconv_wgrad", grad, features.data_ptr(), grad.data_ptr(), book.nbr_out.data_ptr(), book.n_out, book.n_in,
                  book.taps, cin, cout, g_w.data_ptr(), None if g_b is None else g_b.data_ptr(), ws.data_ptr())
        return g_feat, g_w, g_b, None


def sparse_conv(features, weight, bias, book):
    """features (n_in, C_in) float32, weight (C_out, kD, kH, kW, C_in), bias (C_out) or None -> (n_out, C_out) over the
    rulebook.  Differentiable in all three."""
    _chk(features, "features", F32)
    _chk(weight, "weight", F32)
    if bias is not None:
        _chk(bias, "bias", F32)
    if features.dim() != 2 or weight.dim() != 5 or features.shape[1] != weight.shape[-1] or features.shape[0] != book.n_in \
            or tuple(weight.shape[1:4]) != tuple(book.kernel_size):
        raise ValueError("features %s / weight %s do not fit the rulebook (%d rows, kernel %s)"
                         % (tuple(features.shape), tuple(weight.shape), book.n_in, book.kernel_size))
    _check_channels(weight.shape[-1], weight.shape[0])
    return _SparseConvFunction.apply(features, weight, bias, book)


class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape, batch_size, indice_dict=None, num_active=None, status=None):
        """features (N, C) float32, indices (N, 4) int32 (b, z, y, x), spatial_shape (D, H, W).
        num_active: the padded form -- a device int32 of one element; rows [0, *num_active) are live, the rest dead
        (indices -1).  status: the int32 word all tensors of one forward share (made here when absent)."""
        self.features = features
        self.indices = indices
        self.spatial_shape = [int(v) for v in spatial_shape]
        self.batch_size = int(batch_size)
        self.indice_dict = {} if indice_dict is None else indice_dict
        self.num_active = self.status = None
        self.caps = {}          # padded form: indice_key -> rows reserved for that strided convolution's output
        if num_active is not None:
            self.num_active = _count_ok(num_active, "num_active")
            self.status = torch.zeros((1,), dtype=I32, device=num_active.device) if status is None else _count_ok(status, "status")
        elif status is not None:
            raise ValueError("status belongs to a padded tensor: pass num_active too")

    def replace_feature(self, feature):
        """A tensor with other features on the same sites (spconv 2.x); the rulebooks are shared."""
        out = SparseConvTensor(feature, self.indices, self.spatial_shape, self.batch_size, self.indice_dict, self.num_active,
                               self.status)
        out.caps = self.caps
        return out

    def dense(self, channels_first=True):
        """(B, C, D, H, W), zero at inactive sites: the pillar scatter over the sites flattened to (b, 0, z * H + y, x)."""
        D, H, W = self.spatial_shape
        idx = self.indices
        flat = torch.stack([idx[:, 0], torch.zeros_like(idx[:, 0]), idx[:, 1] * H + idx[:, 2], idx[:, 3]], dim=1).contiguous()
        out = pillar_scatter(self.features.contiguous(), flat, self.batch_size, D * H, W, count=self.num_active)
        out = out.view(self.batch_size, self.features.shape[1], D, H, W)
        return out if channels_first else out.permute(0, 2, 3, 4, 1).contiguous()


class _CountedBatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, count, status, eps, momentum, relu, training):
        cap, c = x.shape
        y = torch.empty_like(x)
        stats = torch.empty((2, c), dtype=F32, device=x.device)
        scratch = torch.empty((bn_relu_scratch_bytes(c),), dtype=torch.uint8, device=x.device)
        if training and running_mean is not None:
            _buffers_written(running_mean)
        _call("pda_bn_relu_fwd_counted", x, x.data_ptr(), weight.data_ptr(), bias.data_ptr(),
              None if running_mean is None else running_mean.data_ptr(),
              None if running_var is None else running_var.data_ptr(), y.data_ptr(), stats.data_ptr(), scratch.data_ptr(), cap, c,
              float(eps), float(momentum), count.data_ptr(), status.data_ptr(), int(relu), int(training))
        ctx.save_for_backward(x, weight, bias, stats, count)
        ctx.flags = (int(relu), int(training))
        return y

    @staticmethod
    def backward(ctx, grad):
        x, weight, bias, stats, count = ctx.saved_tensors
        cap, c = x.shape
        grad = grad.contiguous()
        g_x = torch.empty_like(x)
        g_w, g_b = torch.empty_like(weight), torch.empty_like(bias)
        scratch = torch.empty((bn_relu_scratch_bytes(c),), dtype=torch.uint8, device=x.device)
        _call("pda_bn_relu_bwd_counted", x, x.data_ptr(), grad.data_ptr(), weight.data_ptr(), bias.data_ptr(), stats.data_ptr(),
              g_x.data_ptr(), g_w.data_ptr(), g_b.data_ptr(), scratch.data_ptr(), cap, c, count.data_ptr(), ctx.flags[0], ctx.flags[1])
        return (g_x, g_w, g_b) + (None,) * 8


class _CountedBatchNormAddReLU(torch.autograd.Function):
    """relu(bn(x) + identity): _CountedBatchNorm's statistics, one apply pass forward and one backward
    (pda_bn_add_relu_*_counted).  The backward takes its ReLU mask from the saved output."""

    @staticmethod
    def forward(ctx, x, identity, weight, bias, running_mean, running_var, count, status, eps, momentum, training):
        cap, c = x.shape
        y = torch.empty_like(x)
        stats = torch.empty((2, c), dtype=F32, device=x.device)
        scratch = torch.empty((bn_relu_scratch_bytes(c),), dtype=torch.uint8, device=x.device)
        if training and running_mean is not None:
            _buffers_written(running_mean)
        _call("pda_bn_add_relu_fwd_counted", x, x.data_ptr(), identity.data_ptr(), weight.data_ptr(), bias.data_ptr(),
              None if running_mean is None else running_mean.data_ptr(),
              None if running_var is None else running_var.data_ptr(), y.data_ptr(), stats.data_ptr(), scratch.data_ptr(), cap, c,
              float(eps), float(momentum), count.data_ptr(), status.data_ptr(), int(training))
        ctx.save_for_backward(x, y, weight, bias, stats, count)
        ctx.training = int(training)
        return y

    @staticmethod
    def backward(ctx, grad):
        x, y, weight, bias, stats, count = ctx.saved_tensors
        cap, c = x.shape
        grad = grad.contiguous()
        g_x, g_id = torch.empty_like(x), torch.empty_like(x)
        g_w, g_b = torch.empty_like(weight), torch.empty_like(bias)
        scratch = torch.empty((bn_relu_scratch_bytes(c),), dtype=torch.uint8, device=x.device)
        _call("pda_bn_add_relu_bwd_counted", x, x.data_ptr(), y.data_ptr(), grad.data_ptr(), weight.data_ptr(), bias.data_ptr(),
              stats.data_ptr(), g_x.data_ptr(), g_id.data_ptr(), g_w.data_ptr(), g_b.data_ptr(), scratch.data_ptr(), cap, c,
              count.data_ptr(), ctx.training)
        return (g_x, g_id, g_w, g_b) + (None,) * 7


def _counted_bn_mode(bn, x, count, status):
    """The checks of a counted BatchNorm call and the module's mode; in training mode num_batches_tracked moves here."""
    _chk(x, "features", F32)
    _counted_args(count, status)
    if x.dim() != 2 or x.shape[1] != bn.num_features:
        raise ValueError("features %s do not fit BatchNorm1d(%d)" % (tuple(x.shape), bn.num_features))
    if not bn.affine or bn.momentum is None:
        raise NotImplementedError("the counted BatchNorm takes an affine module with a fixed momentum")
    training = bn.training or bn.running_mean is None
    if training and bn.training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return bool(training)


def counted_batch_norm(bn, x, count, status, relu=False):
    """nn.BatchNorm1d `bn` (+ ReLU) over the live rows [0, *count) of x (cap, C) through pda_bn_relu_*_counted, with the
    module's own parameters and buffers: batch statistics in training mode (running statistics and num_batches_tracked
    updated on the device), running statistics in eval mode.  Dead rows of the result and of the gradient are exact zeros.
    Fewer than two live rows in training mode set FLAG_FEW_ROWS in *status where torch would have raised."""
    training = _counted_bn_mode(bn, x, count, status)
    return _CountedBatchNorm.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, count, status, bn.eps, bn.momentum,
                                   bool(relu), training)


def counted_batch_norm_add_relu(bn, x, identity, count, status):
    """relu(bn(x) + identity) over the live rows [0, *count) of x and identity (cap, C), the tail of a residual block, through
    pda_bn_add_relu_*_counted: the bits of counted_batch_norm(relu=False), `+` and ReLU one after the other, forward and
    backward, in one apply pass each.  Mode, buffers, dead rows and FLAG_FEW_ROWS as in counted_batch_norm; dead rows of
    identity are not read."""
    training = _counted_bn_mode(bn, x, count, status)
    _chk(identity, "identity", F32)
    if identity.shape != x.shape:
        raise ValueError("identity %s does not fit the features %s" % (tuple(identity.shape), tuple(x.shape)))
    return _CountedBatchNormAddReLU.apply(x, identity, bn.weight, bn.bias, bn.running_mean, bn.running_var, count, status,
                                          bn.eps, bn.momentum, training)


def padded_report(batch_dict_or_tensor):
    """One host read after a forward of the padded form: ({indice_key or 'input': live rows}, {same: capacity}, status word).
    For choosing PADDED_CAPS and for checking a run at whatever interval the caller likes (status != 0: see the FLAG_*)."""
    x = batch_dict_or_tensor
    if isinstance(x, dict):
        x = x['encoded_spconv_tensor']
    if x.num_active is None:
        raise ValueError("not a padded tensor")
    books = [(key, b) for key, b in x.indice_dict.items() if b.kind == 'spconv' and b.count_out is not None]
    first = next((b for b in x.indice_dict.values() if b.kind == 'subm' and b.count_out is not None), None)
    names = (['input'] if first is not None else []) + [key for key, _ in books]
    words = ([first.count_out] if first is not None else []) + [b.count_out for _, b in books] + [x.status]
    host = torch.cat([w.reshape(1) for w in words]).tolist()                # the one host read
    caps = ([first.n_in] if first is not None else []) + [b.n_out for _, b in books]
    return dict(zip(names, host[:-1])), dict(zip(names, caps)), host[-1]


class SparseModule(nn.Module):
    """Marks a module that takes and returns a SparseConvTensor."""


class SparseSequential(SparseModule):
    """nn.Sequential's child naming (so state-dict keys match); a child that is not a SparseModule is applied to the
    features of a sparse input."""

    def __init__(self, *args):
        super().__init__()
        for i, module in enumerate(args):
            self.add_module(str(i), module)

    def __getitem__(self, idx):
        return list(self._modules.values())[idx]

    def __len__(self):
        return len(self._modules)

    def forward(self, input):
        if isinstance(input, SparseConvTensor) and input.num_active is not None:
            return self._forward_padded(input)
        for module in self._modules.values():
            if isinstance(module, SparseModule):
                input = module(input)
            elif isinstance(input, SparseConvTensor):
                if input.indices.shape[0] != 0:
                    input = input.replace_feature(module(input.features))
            else:
                input = module(input)
        return input

    def _forward_padded(self, input):
        """A BatchNorm1d child runs through the counted kernels on the module's own parameters and buffers, with a directly
        following ReLU folded in; every other child as above (a ReLU keeps the zeros of the dead rows)."""
        mods = list(self._modules.values())
        i = 0
        while i < len(mods):
            module = mods[i]
            i += 1
            if isinstance(module, SparseModule):
                input = module(input)
            elif isinstance(module, nn.BatchNorm1d):
                relu = i < len(mods) and isinstance(mods[i], nn.ReLU)
                input = input.replace_feature(counted_batch_norm(module, input.features, input.num_active, input.status, relu))
                i += 1 if relu else 0
            else:
                input = input.replace_feature(module(input.features))
        return input


class SparseConvolution(SparseModule):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=0, dilation=1, groups=1, bias=True, subm=False,
                 indice_key=None, check=False):
        super().__init__()
        if _triple(dilation, "dilation") != (1, 1, 1) or groups != 1:
            raise NotImplementedError("dilation %r / groups %r: only dilation 1 and groups 1 are implemented" % (dilation, groups))
        _check_channels(in_channels, out_channels)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride = _triple(kernel_size, "kernel_size"), _triple(stride, "stride")
        self.padding, self.dilation, self.groups = _triple(padding, "padding"), (1, 1, 1), 1
        self.subm, self.indice_key, self.check = subm, indice_key, check
        if subm and (self.stride != (1, 1, 1) or any(k % 2 != 1 for k in self.kernel_size)):
            raise NotImplementedError("SubMConv3d takes an odd kernel and stride 1")
        self.weight = nn.Parameter(torch.empty((out_channels,) + self.kernel_size + (in_channels,)))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in = self.in_channels * self.kernel_size[0] * self.kernel_size[1] * self.kernel_size[2]
            bound = 1 / math.sqrt(fan_in)
            nn.init.uniform_(self.bias, -bound, bound)

    def extra_repr(self):
        return "%d, %d, kernel_size=%s, stride=%s, padding=%s, subm=%s, indice_key=%r" % (
            self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding, self.subm, self.indice_key)

    def _rulebook(self, x):
        n = x.indices.shape[0]
        kind = 'subm' if self.subm else 'spconv'
        pad = tuple(k // 2 for k in self.kernel_size) if self.subm else self.padding
        book = None if self.indice_key is None else x.indice_dict.get(self.indice_key)
        if book is not None:
            if not book.matches(kind, self.kernel_size, self.stride, pad, x.spatial_shape, n):
                raise ValueError("indice_key %r was built for another convolution or other input sites" % (self.indice_key,))
            return book
        indices = x.indices if x.indices.dtype == I32 else x.indices.to(I32)
        indices = indices.contiguous()
        if self.subm:
            book = build_subm_rulebook(indices, x.spatial_shape, x.batch_size, self.kernel_size, check=self.check,
                                       count=x.num_active, status=x.status)
        else:
            book = build_strided_rulebook(indices, x.spatial_shape, x.batch_size, self.kernel_size, self.stride, self.padding,
                                          cap=x.caps.get(self.indice_key) if x.num_active is not None else None,
                                          count=x.num_active, status=x.status)
            book.in_indices = indices
        if self.indice_key is not None:
            x.indice_dict[self.indice_key] = book
        return book

    def forward(self, input):
        if not isinstance(input, SparseConvTensor):
            raise TypeError("a sparse convolution takes a SparseConvTensor")
        if not input.features.is_cuda:
            raise RuntimeError("features must be a CUDA(HIP) tensor -- there is no CPU path")
        book = self._rulebook(input)
        features = sparse_conv(input.features.contiguous(), self.weight, self.bias, book)
        out_indices = input.indices if self.subm else book.out_indices
        out = SparseConvTensor(features, out_indices, book.out_shape, input.batch_size, input.indice_dict,
                               None if input.num_active is None else book.count_out, input.status)
        out.caps = input.caps
        return out


class SubMConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None, check=False):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, True, indice_key, check)


class SparseConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, False, indice_key)


class SparseInverseConv3d(SparseModule):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("spconv_utils.SparseInverseConv3d refuses: the inverse convolution is "
                                  "pdanet_amd.spconv_unet.SparseInverseConv3d (UNetV2 builds it there)")


class SparseConvTranspose3d(SparseModule):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("transposed sparse convolutions are not implemented")


def replace_feature(out, new_features):
    return out.replace_feature(new_features)


def find_all_spconv_keys(model, prefix=""):
    """The weight keys of every sparse convolution below `model`: what a caller transposes when it loads a spconv 1.x
    checkpoint (this package keeps the spconv 2.x layout and transposes nothing itself)."""
    found = set()
    for name, child in model.named_children():
        new_prefix = "%s.%s" % (prefix, name) if prefix != "" else name
        if isinstance(child, SparseConvolution):
            new_prefix = "%s.weight" % new_prefix
            found.add(new_prefix)
        found.update(find_all_spconv_keys(child, prefix=new_prefix))
    return found
