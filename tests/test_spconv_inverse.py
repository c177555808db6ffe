"""SparseInverseConv3d (pdanet_amd/spconv_unet.py) against the dense restatement of its contract
(tests/golden/unet_restatement.py: torch.nn.functional.conv_transpose3d masked to the strided convolution's input sites).

CPU part: constructor, weight layout, find_all_spconv_keys, the ValueErrors (raised on CPU tensors, so before any launch), the
refusing stub of spconv_utils, and the restatement against the rulebook statement y[i] = sum_t W'[:, t, :] . x[nbr_in[i][t]].
GPU part: forward, data gradient and weight gradient of sum(y^2) on a (9, 10, 12) grid, 2 x 150 sites, for two strided
rulebooks (even and odd extents: output_padding 0 and 1) and three channel pairs.

Tolerance (the rule of tests/test_second_net.py): the restatement runs in float64 and in float32 on the CPU; the float32 error
against float64 is measured here as max |a - ref| / max |ref|, and the device may be off by FACTOR = 4 times that.  Both
figures are printed; BASELINE.md section 4 records them."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from pdanet_amd import spconv_utils as sp
from pdanet_amd import spconv_unet as un

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import sparse_conv_restatement as rs  # noqa: E402
import unet_restatement as ur  # noqa: E402

gpu = pytest.mark.gpu
GRID, BATCH, PER_SCENE, FACTOR = (9, 10, 12), 2, 150, 4.0
BOOKS = {'s2p1': (3, 2, 1), 's2p011': (3, 2, (0, 1, 1))}
CHANNELS = [(64, 32), (32, 16), (5, 16)]


@functools.lru_cache(maxsize=None)
def sites():
    """(300, 4) int64 rows (b, z, y, x): 150 distinct random cells in each of the two scenes, rows shuffled."""
    D, H, W = GRID
    rng = np.random.default_rng(21)
    rows = []
    for b in range(BATCH):
        cells = rng.choice(D * H * W, PER_SCENE, replace=False)
        rows.append(np.stack([np.full(PER_SCENE, b), cells // (H * W), (cells // W) % H, cells % W], axis=1))
    rows = np.concatenate(rows).astype(np.int64)
    return rows[rng.permutation(len(rows))]


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_constructor_weight_layout_and_spconv_keys():
    conv = un.SparseInverseConv3d(64, 32, 3, indice_key='spconv3', bias=False)
    assert isinstance(conv, sp.SparseConvolution) and tuple(conv.weight.shape) == (32, 3, 3, 3, 64) and conv.bias is None
    assert un.SparseInverseConv3d(5, 16, (3, 1, 1), indice_key='k').bias.shape == (16,)
    seq = sp.SparseSequential(sp.SparseConv3d(16, 32, 3, stride=2, padding=1, indice_key='d'), torch.nn.ReLU(),
                              un.SparseInverseConv3d(32, 16, 3, indice_key='d'))
    assert sp.find_all_spconv_keys(seq) == {'0.weight', '2.weight'}
    with pytest.raises(NotImplementedError):                                # the channel limits of _check_channels
        un.SparseInverseConv3d(16, 24, 3, indice_key='d')
    with pytest.raises(NotImplementedError):
        un.SparseInverseConv3d(129, 16, 3, indice_key='d')
    with pytest.raises(ValueError):
        un.SparseInverseConv3d(16, 16, 3, indice_key=None)


def test_stub_in_spconv_utils_still_refuses():
    with pytest.raises(NotImplementedError, match="spconv_unet"):
        sp.SparseInverseConv3d(16, 16, 3, indice_key='x')


def cpu_book(kind, n_in, n_out):
    i32 = torch.int32
    return sp.Rulebook(kind, (3, 3, 3), (2, 2, 2) if kind == 'spconv' else (1, 1, 1), (1, 1, 1), GRID, [5, 5, 6] if kind == 'spconv'
                       else GRID, n_in, torch.zeros((n_out, 4), dtype=i32), torch.zeros((n_out, 27), dtype=i32),
                       torch.zeros((n_in, 27), dtype=i32) if kind == 'spconv' else None)


def test_value_errors_come_before_any_launch():
    conv = un.SparseInverseConv3d(16, 16, 3, indice_key='d')
    x = sp.SparseConvTensor(torch.zeros(7, 16), torch.zeros(7, 4, dtype=torch.int32), [5, 5, 6], 1)      # CPU tensors throughout
    with pytest.raises(ValueError, match="no rulebook"):
        conv(x)
    x.indice_dict['d'] = cpu_book('subm', 7, 7)
    with pytest.raises(ValueError, match="submanifold"):
        conv(x)
    x.indice_dict['d'] = cpu_book('spconv', 20, 8)                           # 8 output rows, the tensor has 7
    x.indice_dict['d'].in_indices = torch.zeros(20, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="7 rows"):
        conv(x)
    x.indice_dict['d'] = cpu_book('spconv', 20, 7)                           # fits, but built by hand: no input sites kept
    with pytest.raises(ValueError, match="input sites"):
        conv(x)
    x.indice_dict['d'].in_indices = torch.zeros(20, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):                   # all checks passed: only now the device is asked for
        conv(x)
    padded = sp.SparseConvTensor(torch.zeros(7, 16), torch.zeros(7, 4, dtype=torch.int32), [5, 5, 6], 1, x.indice_dict,
                                 num_active=torch.tensor([7], dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="padded"):
        conv(padded)


def test_rulebook_keeps_input_sites_only_when_a_layer_builds_it():
    assert cpu_book('spconv', 3, 2).in_indices is None and cpu_book('subm', 3, 3).in_indices is None


@pytest.mark.parametrize("name", list(BOOKS))
def test_restatement_equals_the_rulebook_statement(name):
    k, s, p = BOOKS[name]
    idx = sites()
    out_idx, nbr_out, nbr_in = rs.rulebook(idx, GRID, BATCH, k, s, p, False)
    rng = np.random.default_rng(4)
    x, w, b = rng.standard_normal((len(out_idx), 5)), rng.standard_normal((16, 3, 3, 3, 5)), rng.standard_normal(16)
    wt = w.reshape(16, 27, 5)
    want = sum(np.where((nbr_in[:, t] >= 0)[:, None], x[nbr_in[:, t]] @ wt[:, t].T, 0) for t in range(27)) + b
    got = ur.inverse_conv_rows(torch.tensor(x), out_idx, idx, GRID, BATCH, torch.tensor(w), torch.tensor(b), k, s, p)
    assert np.abs(got.numpy() - want).max() < 1e-12
    # both output_padding cases occur: the even extents (10, 12) leave one cell for it, the odd one (9) none
    k3, s3, p3 = rs.triple(k), rs.triple(s), rs.triple(p)
    assert ur.output_padding(GRID, rs.out_shape(GRID, k3, s3, p3), k3, s3, p3) == (0, 1, 1)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def device_case(name, cin, cout, x, w, b):
    """The strided layer builds the rulebook; the inverse layer runs on features x placed on its output sites.  Returns the
    output tensor, the rulebook, and y, dL/dx, dL/dW', dL/db of L = sum(y^2) as numpy."""
    k, s, p = BOOKS[name]
    idx = sites()
    down = sp.SparseConv3d(4, 16, k, stride=s, padding=p, bias=False, indice_key='d').cuda()
    inv = un.SparseInverseConv3d(cin, cout, k, indice_key='d', bias=b is not None).cuda()
    with torch.no_grad():
        inv.weight.copy_(dev(w))
        if b is not None:
            inv.bias.copy_(dev(b))
    x0 = sp.SparseConvTensor(torch.zeros(len(idx), 4, device='cuda'), dev(idx, torch.int32), GRID, BATCH)
    mid = down(x0)
    xt = dev(x).requires_grad_(True)
    y = inv(mid.replace_feature(xt))
    (y.features ** 2).sum().backward()
    torch.cuda.synchronize()
    g = lambda t: None if t is None else t.grad.cpu().numpy()
    return y, x0.indice_dict['d'], [y.features.detach().cpu().numpy(), g(xt), g(inv.weight), g(inv.bias)]


def restated(name, x, w, b, out_idx, dtype):
    k, s, p = BOOKS[name]
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    wt = torch.tensor(w, dtype=dtype, requires_grad=True)
    bt = None if b is None else torch.tensor(b, dtype=dtype, requires_grad=True)
    y = ur.inverse_conv_rows(xt, out_idx, sites(), GRID, BATCH, wt, bt, k, s, p)
    (y ** 2).sum().backward()
    return [y.detach().numpy(), xt.grad.numpy(), wt.grad.numpy(), None if bt is None else bt.grad.numpy()]


@gpu
@pytest.mark.parametrize("name", list(BOOKS))
@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_gpu_inverse_conv_forward_and_gradients(name, cin, cout):
    k, s, p = BOOKS[name]
    idx = sites()
    out_idx, _ = rs.output_sites(idx, GRID, BATCH, k, s, p)
    rng = np.random.default_rng(300 + cin + cout + len(name))
    x = rng.standard_normal((len(out_idx), cin)).astype(np.float32)
    w = (rng.standard_normal((cout, 3, 3, 3, cin)) * 0.05).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32) if cin == 32 else None
    y, book, got = device_case(name, cin, cout, x, w, b)
    # the sites: the strided convolution's input sites, row for row, on its input grid
    assert np.array_equal(book.out_indices.cpu().numpy(), out_idx) and book.n_in == len(idx)
    assert np.array_equal(y.indices.cpu().numpy(), idx) and y.spatial_shape == list(GRID) and y.features.shape == (len(idx), cout)
    assert y.indice_dict['d'] is book
    ref = restated(name, x, w, b, out_idx, torch.float64)
    f32 = restated(name, x, w, b, out_idx, torch.float32)
    for what, d, c, r in zip(("forward", "data gradient", "weight gradient", "bias gradient"), got, f32, ref):
        if r is None:
            assert d is None
            continue
        e_dev, e_f32 = rel(d, r), rel(c, r)
        print("inverse", name, cin, cout, what, "device err", e_dev, "float32 CPU err", e_f32)
    for what, d, c, r in zip(("forward", "data gradient", "weight gradient", "bias gradient"), got, f32, ref):
        if r is not None:
            assert rel(d, r) <= FACTOR * rel(c, r), what
    # two runs give the same bits
    _, _, again = device_case(name, cin, cout, x, w, b)
    for a, c in zip(got, again):
        assert (a is None and c is None) or a.tobytes() == c.tobytes()


@gpu
def test_gpu_inverse_conv_exact_on_small_integers():
    """Every product and partial sum is an integer below 2^24: any order on the exact f32 MFMA gives float64's bits."""
    name, cin, cout = 's2p011', 5, 16
    k, s, p = BOOKS[name]
    out_idx, _ = rs.output_sites(sites(), GRID, BATCH, k, s, p)
    rng = np.random.default_rng(8)
    x = rng.integers(-4, 5, (len(out_idx), cin)).astype(np.float32)
    w = rng.integers(-4, 5, (cout, 3, 3, 3, cin)).astype(np.float32)
    b = rng.integers(-4, 5, cout).astype(np.float32)
    _, _, got = device_case(name, cin, cout, x, w, b)
    ref = restated(name, x, w, b, out_idx, torch.float64)
    for d, r in zip(got, ref):
        assert np.abs(r).max() < 2 ** 24 and np.array_equal(d.astype(np.float64), r)


@gpu
def test_gpu_inverse_conv_refuses_a_book_without_input_sites_and_other_rows():
    idx = sites()
    ind = dev(idx, torch.int32)
    book = sp.build_strided_rulebook(ind, GRID, BATCH, 3, 2, 1)             # built by hand: in_indices stays None
    inv = un.SparseInverseConv3d(16, 16, 3, indice_key='d').cuda()
    x = sp.SparseConvTensor(torch.zeros(book.n_out, 16, device='cuda'), book.out_indices, book.out_shape, BATCH, {'d': book})
    with pytest.raises(ValueError, match="input sites"):
        inv(x)
    book.in_indices = ind
    assert inv(x).features.shape == (len(idx), 16)
    short = sp.SparseConvTensor(torch.zeros(book.n_out - 1, 16, device='cuda'), book.out_indices[:-1], book.out_shape, BATCH, {'d': book})
    with pytest.raises(ValueError, match="rows"):
        inv(short)
