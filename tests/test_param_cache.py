"""pdanet_amd/param_cache.py on CPU tensors with a counting `make`: the stamp, the two writers and the store's three
validity conditions (stamp, owner alive, owner still at the address)."""
import gc

import pytest
import torch
import torch.nn as nn

import pdanet_amd
from pdanet_amd import param_cache


class Make:
    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return object()


@pytest.mark.parametrize("weights_only", [False, True])
def test_hit_while_unchanged_and_miss_after_each_writer(weights_only):
    store, make = param_cache.Store(under_capture=False, weights_only=weights_only), Make()
    p = nn.Parameter(torch.randn(8, 4))
    get = lambda: store.get(p, (p,), make)
    a = get()
    assert get() is a and get() is a and make.calls == 1
    with torch.no_grad():
        p.mul_(0.5)                                        # an in-place write moves the version counter
    b = get()
    assert b is not a and get() is b and make.calls == 2
    param_cache.parameters_written()
    c = get()
    assert c is not b and get() is c and make.calls == 3
    param_cache.buffers_written()
    d = get()
    if weights_only:                                        # planes packed in a forward pass outlive the BN kernels of that pass
        assert d is c and make.calls == 3
    else:
        assert d is not c and get() is d and make.calls == 4


def test_data_write_is_not_seen_until_reported():
    """`p.data.mul_()` moves neither the version counter nor an epoch: the entry still hits.  This is pinned, not wished
    for -- whoever writes through `.data` or a raw pointer calls pdanet_amd.invalidate_weight_caches()."""
    store, make = param_cache.Store(under_capture=False), Make()
    p = nn.Parameter(torch.randn(8, 4))
    a = store.get(p, (p,), make)
    p.data.mul_(0.5)
    assert store.get(p, (p,), make) is a and make.calls == 1
    assert pdanet_amd.invalidate_weight_caches is param_cache.parameters_written
    pdanet_amd.invalidate_weight_caches()
    assert store.get(p, (p,), make) is not a and make.calls == 2


def test_every_source_counts():
    """A buffer replaced by a different tensor with the same version counter (0 after .cuda(), 0 for a fresh torch.full)."""
    store, make = param_cache.Store(under_capture=True), Make()
    bn = nn.BatchNorm1d(16)
    bn.running_var = torch.full((16,), 1.0)
    w = nn.Parameter(torch.randn(16, 4))
    a = store.get(bn, (w, bn.running_mean, bn.running_var), make)
    assert store.get(bn, (w, bn.running_mean, bn.running_var), make) is a
    old, bn.running_var = bn.running_var, torch.full((16,), 4.0)      # (`old` keeps the address from being reused)
    assert bn.running_var._version == old._version
    assert store.get(bn, (w, bn.running_mean, bn.running_var), make) is not a and make.calls == 2
    assert param_cache.stamp((w, None))[2] is None


def test_owner_collected_and_address_reused():
    store, make = param_cache.Store(under_capture=False, weights_only=True), Make()
    q = None
    for _ in range(16):                                     # (whether malloc hands a freed block out again varies: 16 x 4 tries)
        p = nn.Parameter(torch.randn(64, 32))
        addr, calls = p.data_ptr(), make.calls
        a = store.get_at(p, make)
        assert len(store) == 1 and make.calls == calls + 1
        del p
        gc.collect()
        assert len(store) == 0                              # dropped with its owner; no strong reference held it
        for _ in range(4):
            q = nn.Parameter(torch.empty(64, 32))
            if q.data_ptr() == addr:
                break
            q = None
        if q is not None:
            break
    else:
        pytest.skip("the allocator never handed a freed address out again in 64 tries")
    calls = make.calls
    assert store.get_at(q.detach(), make) is None           # same address, version and epoch: still no hit
    b = store.get_at(q, make)
    assert b is not a and make.calls == calls + 1


def test_repointed_owner_misses_at_both_addresses():
    store, make = param_cache.Store(under_capture=False, weights_only=True), Make()
    p = nn.Parameter(torch.randn(8, 4))
    old, other = p.detach(), torch.randn(8, 4)
    a = store.get_at(p, make)
    assert store.get_at(old, make) is a                     # an alias finds it by address
    p.data = other
    assert store.get_at(old, make) is None                  # the owner no longer sits there
    assert store.get_at(other, make) is None
    assert make.calls == 1


def test_address_lookup_through_views():
    store, make = param_cache.Store(under_capture=False, weights_only=True), Make()
    conv = nn.Conv2d(4, 8, 1)
    w2d = conv.weight.flatten(1)
    assert param_cache.owning_parameter(w2d) is conv.weight and param_cache.owning_parameter(conv.weight) is conv.weight
    a = store.get_at(w2d, make, extra=(8, 4))
    saved = w2d.detach()                                    # what a backward pass holds: an alias without an owner
    assert param_cache.owning_parameter(saved) is None
    assert store.get_at(saved, make, extra=(8, 4)) is a
    assert store.get_at(conv.weight.flatten(1), make, extra=(8, 4)) is a

    w = nn.Parameter(torch.randn(12, 4))
    rows = w[4:8]
    assert rows.is_contiguous() and param_cache.owning_parameter(rows) is w
    b = store.get_at(rows, make, extra=(4, 4))
    assert store.get_at(rows.detach(), make, extra=(4, 4)) is b
    assert store.get_at(w[4:8], make, extra=(4, 4)) is b and make.calls == 2
    with torch.no_grad():
        w.mul_(2.0)                                         # the view shares the Parameter's version counter
    assert store.get_at(rows.detach(), make, extra=(4, 4)) is None

    loose = torch.randn(8, 4)                               # no owning Parameter: never stored
    n = len(store)
    assert store.get_at(loose, make) is None
    assert len(store) == n and make.calls == 2
