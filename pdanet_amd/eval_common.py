"""Host-side plumbing shared by the device evaluations (once_eval.py, kitti_eval.py): the one-copy upload and the
workspace (stage_common.py's, shared with the data stages), the name table, post_processing's label-to-name rule, the
frame row bookkeeping and the layout of the one int64 result buffer.
What is dataset-specific (class and accept tables, frame modes, the AP composition) stays in the two modules.
"""
import numpy as np
import torch

from .stage_common import upload, workspace  # noqa: F401  (the evaluations upload pageable: upload(arrays, device))


def ptr(t):
    """The device address of a tensor, null for None or an empty one."""
    return t.data_ptr() if t is not None and t.numel() else None


def vocab(name_lists, max_names, what):
    """name -> id in order of first appearance over the lists; what names the dataset in the size error."""
    ids = {}
    for names in name_lists:
        for n in names:
            ids.setdefault(n, len(ids))
    if len(ids) > max_names:
        raise ValueError("%s evaluation supports at most %d distinct names, got %d" % (what, max_names, len(ids)))
    return ids


def label_name_ids(pred_labels, n_classes):
    """int32 ids of numpy's class_names[label - 1]: label 0 wraps to the last class, a label out of range gives -1."""
    idx = pred_labels.to(torch.int64) - 1
    idx = torch.where(idx < 0, idx + n_classes, idx)
    return torch.where((idx >= 0) & (idx < n_classes), idx, torch.full_like(idx, -1)).to(torch.int32)


def clamp_num_pred(num_pred, capacity):
    """int32 num_pred within [0, capacity], the padded rows of a frame."""
    return torch.clamp(num_pred.to(torch.int32), 0, capacity)


def row_starts(rows):
    """int64 start[f] of frames stored back to back, rows[f] rows each."""
    start = np.zeros(len(rows), np.int64)
    np.cumsum(rows[:-1], out=start[1:])
    return start


def padded_rows(shapes):
    """int64 row length of every frame of padded batches: capacity K for each of the B frames of every (B, K)."""
    return np.concatenate([np.full(B, K, np.int64) for B, K in shapes]) if shapes else np.zeros(0, np.int64)


def pair_offsets(n_gt, rows):
    """(start, total): the first element of each frame's n_gt[f] x rows[f] block of pairs, and their number."""
    starts = np.zeros(len(n_gt) + 1, np.int64)
    np.cumsum(n_gt.astype(np.int64) * rows, out=starts[1:])
    return starts[:-1], int(starts[-1])


class ResultLayout:
    """One int64 result buffer: 8-byte segments (name, dtype, shape) back to back, int64 or float64, then the int32
    status in the last int64.  The kernels write through device_views(), the caller reads through host_views()."""

    def __init__(self, what, segments):
        self.what = what
        self.segments = [(name, np.dtype(dtype), tuple(shape), int(np.prod(shape))) for name, dtype, shape in segments]
        self.total = sum(count for *_, count in self.segments) + 1

    def _split(self, buf, f64):
        views, o = {}, 0
        for name, dtype, shape, count in self.segments:
            views[name] = buf[o:o + count].view(f64) if dtype == np.float64 else buf[o:o + count]
            o += count
        return views

    def alloc(self, device):
        return torch.zeros(self.total, dtype=torch.int64, device=device)

    def device_views(self, res):
        """Flat device views of the segments by name, and 'status' (1) int32."""
        views = self._split(res, torch.float64)
        views['status'] = res[-1:].view(torch.int32)
        return views

    def host_views(self, h):
        """The segments of the host copy h by name, in their shapes; raises on a status bit."""
        status = int(h[-1:].view(np.int32)[0])
        if status:
            raise RuntimeError("%s evaluation: inconsistent inputs (status %d: 1 frame bounds, 2 unknown name id, "
                               "4 too many thresholds)" % (self.what, status))
        views = self._split(h, np.float64)
        return {name: views[name].reshape(shape) for name, _, shape, _ in self.segments}
