"""Host-side plumbing shared by the device data stages (data_processor.py, data_augmentor.py, frame_stage.py,
voxel_utils.py) and, for the upload and the workspace, by the device evaluations (eval_common.py): ragged scenes as
packed rows + offsets + n_cap, the one-copy upload, the workspace of an entry point, and the status column of info.
Its device-side counterpart is csrc/ragged_scene.h.  What a stage does with its scenes stays in its module.
"""
import numpy as np
import torch

from . import _lib

# info[:, 3] status bits every stage shares (include/pda_train.h; csrc/ragged_scene.h)
STATUS_BAD_OFFSETS, STATUS_OVER_CAP = 2, 4

_TORCH_DTYPE = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32,
                np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32}


def cfg_get(cfg, key, default=None):
    return cfg[key] if key in cfg else default


def current_device():
    return torch.device('cuda', torch.cuda.current_device())


def offsets_of(sizes):
    """int64 (len + 1) offsets of rows stored back to back, sizes[i] rows each: a leading zero, then the running sum."""
    offs = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(np.asarray(sizes, np.int64), out=offs[1:])
    return offs


def pack_scenes(arrays):
    """A list of (n_i, C) host arrays -> (packed (n_total, C) float32, offsets (B + 1) int64, n_cap, C)."""
    arrs = [np.asarray(a.numpy() if isinstance(a, torch.Tensor) else a, np.float32) for a in arrays]
    if not arrs:
        raise ValueError("empty batch")
    C = arrs[0].shape[1] if arrs[0].ndim == 2 else -1
    if any(a.ndim != 2 or a.shape[1] != C for a in arrs):
        raise ValueError("every scene must be (n_i, C) with the same C")
    sizes = [a.shape[0] for a in arrs]
    packed = np.concatenate(arrs, 0) if sum(sizes) else np.zeros((0, C), np.float32)
    return packed, offsets_of(sizes), max(max(sizes), 1), C


def packed_form(points):
    """The (packed (n_total, C) float32, offsets (B + 1) int64, n_cap) tuple of device tensors -> (packed, offsets, n_cap)."""
    pts, offs, n_cap = points
    if not (pts.is_cuda and offs.is_cuda):
        raise ValueError("the (packed, offsets, n_cap) form takes device tensors")
    return pts, offs, int(n_cap)


def upload(parts, device, pinned=False):
    """Host arrays (float32 / float64 / int32 / int64, any may be empty) -> device views with their dtypes and shapes,
    through one host buffer and one copy; sections start on 16 bytes (the float4 paths of csrc/frame_stage.hip test for
    it).  pinned: a pinned buffer and an asynchronous copy, else a pageable buffer and a blocking one."""
    parts = [np.ascontiguousarray(p) for p in parts]
    starts, total = [], 0
    for p in parts:
        starts.append(total)
        total += (p.nbytes + 15) // 16 * 16
    host = torch.empty((max(total, 16),), dtype=torch.uint8, pin_memory=pinned)
    hn = host.numpy()
    for p, s in zip(parts, starts):
        hn[s:s + p.nbytes] = p.reshape(-1).view(np.uint8)
    dbuf = host.to(device, non_blocking=pinned)
    return [dbuf[s:s + p.nbytes].view(_TORCH_DTYPE[p.dtype]).view(p.shape) for p, s in zip(parts, starts)]


def workspace(entry, sizes, message, device):
    """The uint8 workspace of a stage: entry = its pda_*_workspace_bytes, which answers -1 for sizes out of range."""
    nbytes = getattr(_lib.load(), entry)(*sizes)
    if nbytes < 0:
        raise ValueError(message)
    return torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=device)


def raise_on_status(info_host, rules, what="scene"):
    """info_host: the (B, 4) host copy of a stage's info.  rules: (mask, message) in the order they are tested; the
    message is what follows "<what> <index>".  Raises ValueError for the first rule the lowest flagged scene matches."""
    for b, status in enumerate(info_host[:, 3].tolist()):
        for mask, message in rules if status else ():
            if status & mask:
                raise ValueError("%s %d%s" % (what, b, message))
