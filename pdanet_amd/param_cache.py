"""When is a tensor that was computed from model parameters still valid?  The one place that answers it.

Derived tensors (bf16 copies and packed bf16 planes of the weights, eval BatchNorm folded into the preceding
convolution, the packed parameter blocks of the fused inference kernels, the captured inference tail) are re-made when
their sources change.  A source has changed when its address or its version counter moved -- or when somebody who wrote it
WITHOUT moving either says so:

  parameters_written()   trained parameters were written through `.data` or a raw pointer (the flat-buffer optimizer
                         step, a broadcast of the flat buffer, a checkpoint copied into it)
  buffers_written()      BatchNorm running statistics were written through a raw pointer (the training-mode BN kernels)

There are two epochs because training forwards write running statistics many times per step, while the weight planes
packed in a forward pass must still hit in the backward pass of the same iteration: entries derived from weights alone
(`weights_only`) key on WEIGHT_EPOCH, which only parameters_written() moves; everything else keys on PARAM_EPOCH, which
both move.  A `.data` write that nobody reports is not seen (tests/test_param_cache.py pins this); callers outside the
package report it with pdanet_amd.invalidate_weight_caches().

An entry of a Store is valid while (1) its stamp matches, (2) its owner -- the Parameter or Module it was derived from --
is alive and (3), for entries found by address, the owner still sits at that address: then no other tensor can occupy
it.  The store holds its owners weakly and drops an entry with its owner, so a freed model whose addresses are reused, or
a Parameter re-pointed by `p.data = ...` (optimization.FlatAdamOneCycle moves the parameters into its flat buffer), never
hits.

Not covered: a replayed TRAINING graph updates running statistics with no Python running, so nothing calls
buffers_written(); staleness there relies on the bump of the optimizer step that follows every replay.
"""
import weakref

import torch
import torch.nn as nn

from . import _lib


def parameters_written():
    _lib.PARAM_EPOCH[0] += 1
    _lib.WEIGHT_EPOCH[0] += 1


def buffers_written():
    _lib.PARAM_EPOCH[0] += 1


def stamp(tensors, weights_only=False):
    """What an entry derived from `tensors` is compared by: the epoch and (address, version counter) of every source."""
    key = [_lib.WEIGHT_EPOCH[0] if weights_only else _lib.PARAM_EPOCH[0]]
    for t in tensors:           # (a plain loop: this runs a few hundred times per step, and a comprehension costs a frame)
        key.append(None if t is None else (t.data_ptr(), t._version))
    return tuple(key)


def owning_parameter(t):
    """The Parameter that `t` is, or is a view of (conv.weight.flatten(1), a slice of in_proj_weight); else None."""
    if isinstance(t, nn.Parameter):
        return t
    base = t._base
    return base if isinstance(base, nn.Parameter) else None


class Store:
    """{key: (stamp, weak reference to the owner, byte offset, value)}.

    under_capture=False: get() neither reads nor fills while the stream is capturing and returns None -- the caller
    records the cast or pack INSIDE the graph, because the training graphs replay across optimizer steps and a replay must
    see the new weights.  True: used as anywhere else -- the inference graph is keyed on the state of the weights and its
    warm-up fills the entries."""

    def __init__(self, under_capture, weights_only=False):
        self.under_capture, self.weights_only = under_capture, weights_only
        self._entries = {}

    def __len__(self):
        return len(self._entries)

    def _collected(self, key, ref):
        ent = self._entries.get(key)
        if ent is not None and ent[1] is ref:
            del self._entries[key]

    def _fill(self, key, st, owner, offset, make):
        value = make()
        self._entries[key] = (st, weakref.ref(owner, lambda r: self._collected(key, r)), offset, value)
        return value

    def get(self, owner, sources, make):
        """The value derived from `sources` for `owner`, from make() on a miss."""
        if not self.under_capture and sources[0].is_cuda and torch.cuda.is_current_stream_capturing():
            return None
        st, key = stamp(sources, self.weights_only), id(owner)
        ent = self._entries.get(key)
        if ent is not None and ent[0] == st and ent[1]() is owner:
            return ent[3]
        return self._fill(key, st, owner, 0, make)

    def get_at(self, t, make, extra=()):
        """The value derived from the tensor `t`, keyed on its storage address: a caller holding only an alias of the owner
        (the backward pass sees a weight as an unpacked saved tensor) finds what was filled through the Parameter or a view of
        it.  The owner is the Parameter that `t` is or views; without one nothing is stored and a miss returns None.  `extra`
        joins the stamp (the shape the address is read with)."""
        if not self.under_capture and t.is_cuda and torch.cuda.is_current_stream_capturing():
            return None
        st = stamp((t,), self.weights_only) + extra
        key = st[1][0]
        ent = self._entries.get(key)
        if ent is not None:
            held = ent[1]()
            if held is None or held.data_ptr() + ent[2] != key:
                del self._entries[key]                    # the owner is gone or lives elsewhere now
            elif ent[0] == st:
                return ent[3]
        owner = owning_parameter(t)
        return None if owner is None else self._fill(key, st, owner, key - owner.data_ptr(), make)
