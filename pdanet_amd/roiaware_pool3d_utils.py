"""Mirror of the part of pcdet/ops/roiaware_pool3d the IA-SSD head uses
(roiaware_pool3d_utils.py:30-43 points_in_boxes_gpu over roiaware_pool3d_cuda.points_in_boxes_gpu,
src/roiaware_pool3d.cpp:98-118) on libpda_pointnet2.so (include/pda_train.h)."""
import torch

from .pointnet2_batch_cuda import F32, I32, _call, _chk, _numel_ok


class roiaware_pool3d_cuda:  # noqa: N801  (the reference's extension module name)
    @staticmethod
    def points_in_boxes_gpu(boxes, pts, box_idx_of_points):
        """(B,T,7) boxes, (B,M,3) points, (B,M) int32 pre-filled with -1 -> 1."""
        b, t, m = boxes.shape[0], boxes.shape[1], pts.shape[1]
        _numel_ok(boxes, b * t * 7, "boxes"); _numel_ok(pts, b * m * 3, "pts")
        _numel_ok(box_idx_of_points, b * m, "box_idx_of_points")
        _call("pda_points_in_boxes", pts, _chk(boxes, "boxes", F32), _chk(pts, "pts", F32),
              _chk(box_idx_of_points, "box_idx_of_points", I32), b, t, m)
        return 1

    @staticmethod
    def forward(rois, pts, pts_feature, argmax, pts_idx_of_voxels, pooled_features, pool_method):
        """roiaware_pool3d.cpp:29-66: rois (N,7), pts (P,3), pts_feature (P,C); the three outputs zero-filled by the caller,
        sizes taken from the tensors.  pool_method 0 max, 1 avg -> 1."""
        n, p, c = rois.shape[0], pts.shape[0], pts_feature.shape[1]
        ox, oy, oz, k = (int(v) for v in pts_idx_of_voxels.shape[1:5])
        _numel_ok(rois, n * 7, "rois"); _numel_ok(pts, p * 3, "pts"); _numel_ok(pts_feature, p * c, "pts_feature")
        _numel_ok(argmax, n * ox * oy * oz * c, "argmax"); _numel_ok(pooled_features, n * ox * oy * oz * c, "pooled_features")
        _numel_ok(pts_idx_of_voxels, n * ox * oy * oz * k, "pts_idx_of_voxels")
        _call("pda_roiaware_pool3d_fwd", pts_feature, _chk(rois, "rois", F32), _chk(pts, "pts", F32),
              _chk(pts_feature, "pts_feature", F32), _chk(argmax, "argmax", I32), _chk(pts_idx_of_voxels, "pts_idx_of_voxels", I32),
              _chk(pooled_features, "pooled_features", F32), n, p, c, k, ox, oy, oz, int(pool_method))
        if p == 0 and int(pool_method) == 0:
            argmax.fill_(-1)                       # the library leaves an empty problem alone; every voxel is empty
        return 1

    @staticmethod
    def backward(pts_idx_of_voxels, argmax, grad_out, grad_in, pool_method):
        """roiaware_pool3d.cpp:68-96: grad_in (P,C), zero-filled by the caller, receives the gradient -> 1."""
        n, ox, oy, oz, k = (int(v) for v in pts_idx_of_voxels.shape)
        c, p = int(grad_out.shape[4]), int(grad_in.shape[0])
        _numel_ok(argmax, n * ox * oy * oz * c, "argmax"); _numel_ok(grad_out, n * ox * oy * oz * c, "grad_out")
        _numel_ok(pts_idx_of_voxels, n * ox * oy * oz * k, "pts_idx_of_voxels"); _numel_ok(grad_in, p * c, "grad_in")
        _call("pda_roiaware_pool3d_bwd", grad_out, _chk(pts_idx_of_voxels, "pts_idx_of_voxels", I32), _chk(argmax, "argmax", I32),
              _chk(grad_out, "grad_out", F32), _chk(grad_in, "grad_in", F32), n, p, c, k, ox, oy, oz, int(pool_method))
        return 1

    @staticmethod
    def points_in_boxes_cpu(boxes, pts, pts_indices):
        """roiaware_pool3d.cpp:143-168 on the device: boxes (N,7), pts (P,3) -> pts_indices (N,P) int32 of 0 / 1 -> 1."""
        n, p = boxes.shape[0], pts.shape[0]
        _numel_ok(boxes, n * 7, "boxes"); _numel_ok(pts, p * 3, "pts"); _numel_ok(pts_indices, n * p, "pts_indices")
        _call("pda_points_in_boxes_mask", pts, _chk(boxes, "boxes", F32), _chk(pts, "pts", F32),
              _chk(pts_indices, "pts_indices", I32), n, p)
        return 1


def points_in_boxes_count(points, boxes):
    """MI355X extension (csrc/roi_pool.hip): what SECONDNetIoU's num_pts_iou_cls score does on the CPU in every scene
    (points_in_boxes_cpu(...).sum(dim=1)), for the batch in one launch and without the boxes x points mask.
    points (N, 1 + 3 + C) float32 [batch, x, y, z, ...] in any order, boxes (B, M, >= 7) float32 -> counts (B, M) int32 of
    the points of scene b inside box (b, m), by the host statement of the test (margin 1e-2, no FMA).  A point whose batch
    value is outside [0, B) counts nowhere."""
    if points.dim() != 2 or points.shape[1] < 4 or boxes.dim() != 3 or boxes.shape[2] < 7:
        raise ValueError("points must be (N, >= 4) and boxes (B, M, >= 7), got %s and %s" % (tuple(points.shape), tuple(boxes.shape)))
    points = points.detach().contiguous()
    boxes = boxes.detach()[..., :7].contiguous()
    B, M = boxes.shape[0], boxes.shape[1]
    counts = torch.zeros((B, M), dtype=I32, device=boxes.device)
    _call("pda_points_in_boxes_count", boxes, _chk(points, "points", F32), int(points.shape[1]), _chk(boxes, "boxes", F32),
          _chk(counts, "counts", I32), int(points.shape[0]), B, M)
    return counts


def points_in_boxes_gpu(points, boxes):
    """
    :param points: (B, M, 3)
    :param boxes: (B, T, 7), num_valid_boxes <= T
    :return box_idxs_of_pts: (B, M), default background = -1
    """
    assert boxes.shape[0] == points.shape[0]
    assert boxes.shape[2] == 7 and points.shape[2] == 3
    batch_size, num_points, _ = points.shape
    box_idxs_of_pts = points.new_zeros((batch_size, num_points), dtype=torch.int).fill_(-1)
    roiaware_pool3d_cuda.points_in_boxes_gpu(boxes.contiguous(), points.contiguous(), box_idxs_of_pts)
    return box_idxs_of_pts


def assign_point_targets(gt_boxes, in_box, in_ext, mode, single_class):
    """MI355X extension (csrc/head_targets.hip): the point-wise part of IASSD_head.assign_stack_targets_IASSD after the two
    points_in_boxes queries, one launch.  gt_boxes (B,T,8), in_box / in_ext (B,N) int32 -> labels (B*N) int64,
    box index (B*N) int64, gt_of_points (B*N,8)."""
    B, T = gt_boxes.shape[0], gt_boxes.shape[1]
    N = in_box.shape[1]
    _numel_ok(gt_boxes, B * T * 8, "gt_boxes"); _numel_ok(in_ext, B * N, "in_ext")
    labels = torch.empty((B * N,), dtype=torch.int64, device=gt_boxes.device)
    idx = torch.empty((B * N,), dtype=torch.int64, device=gt_boxes.device)
    gt_of = torch.empty((B * N, 8), dtype=torch.float32, device=gt_boxes.device)
    _call("pda_assign_point_targets", gt_boxes, _chk(gt_boxes, "gt_boxes", F32), _chk(in_box, "in_box", I32), _chk(in_ext, "in_ext", I32),
          _chk(labels, "labels", torch.int64), _chk(idx, "box_idx", torch.int64), _chk(gt_of, "gt_of_points", F32), B, N, T, int(mode),
          int(bool(single_class)))
    return labels, idx, gt_of


def head_assign_targets(points, gt_boxes, extra_width, mode, single_class, mean_size=None, bins=0, ret_box_labels=False):
    """MI355X extension (csrc/head_targets.hip): assign_stack_targets_IASSD for one point set in ONE launch.  points (B*N, 4)
    [bs, x, y, z] scene-major, gt_boxes (B, T, 8), extra_width 3 python floats -> labels (B*N) int64, box index (B*N) int64,
    gt_of_points (B*N, 8), box-coder targets (B*N, 8) or None."""
    import ctypes
    B, T = gt_boxes.shape[0], gt_boxes.shape[1]
    P = points.shape[0]
    N = P // B
    dev = gt_boxes.device
    labels = torch.empty((P,), dtype=torch.int64, device=dev)
    idx = torch.empty((P,), dtype=torch.int64, device=dev)
    gt_of = torch.empty((P, 8), dtype=torch.float32, device=dev)
    box_labels = torch.empty((P, 8), dtype=torch.float32, device=dev) if ret_box_labels else None
    ew = (ctypes.c_float * 3)(*[float(w) for w in extra_width])
    _call("pda_head_assign_targets", gt_boxes, _chk(points, "points", F32), int(points.shape[1]), 1, _chk(gt_boxes, "gt_boxes", F32), ew,
          _chk(labels, "labels", torch.int64), _chk(idx, "box_idx", torch.int64), _chk(gt_of, "gt_of_points", F32),
          None if box_labels is None else _chk(box_labels, "box_labels", F32), None if mean_size is None else _chk(mean_size, "mean_size", F32),
          int(bins), B, N, T, int(mode), int(bool(single_class)))
    return labels, idx, gt_of, box_labels


def sa_gaussian_mask(coords, gt_of_points, labels):
    """MI355X extension: soft instance labels (IASSD_head.py:889-963) for the points coords (P, 1+3[+...]) [bs, x, y, z, ...]
    against their boxes gt_of_points (P, 8); 0 where labels <= 0.  One launch."""
    P = gt_of_points.shape[0]
    _numel_ok(coords, P * coords.shape[-1], "coords"); _numel_ok(labels, P, "labels")
    out = torch.empty((P,), dtype=torch.float32, device=gt_of_points.device)
    _call("pda_sa_gaussian_mask", gt_of_points, _chk(coords, "coords", F32), int(coords.shape[-1]), 1, _chk(gt_of_points, "gt_of_points", F32),
          _chk(labels, "labels", torch.int64), _chk(out, "out", F32), P)
    return out


# ---- loss terms of the IA-SSD head, one launch each (csrc/head_loss.hip) ------------------------------------------------------
I64 = torch.int64


def head_centerness(centers, gt_of_points, labels):
    """generate_center_ness_mask (IASSD_head.py:795-817): centers (n, 4) [bs, x, y, z], gt (n, 8), labels (n) -> (n)."""
    n = gt_of_points.shape[0]
    out = torch.empty((n,), dtype=torch.float32, device=gt_of_points.device)
    _call("pda_head_centerness", gt_of_points, _chk(centers, "centers", F32), _chk(gt_of_points, "gt_of_points", F32),
          _chk(labels, "labels", I64), _chk(out, "out", F32), n)
    return out


class _ScaledGrad(torch.autograd.Function):
    """Shared shape of the fused loss nodes: forward(prediction tensors..., run) calls `run()`, which launches the kernel and
    returns (outputs, gradients of the term wrt each prediction tensor); backward multiplies the stored gradients by the
    incoming scalar of output 0 (the other outputs are logged values without gradient)."""

    @staticmethod
    def forward(ctx, run, *preds):
        outs, grads = run()
        ctx.save_for_backward(*grads)
        ctx.mark_non_differentiable(*outs[1:])
        return tuple(outs)

    @staticmethod
    def backward(ctx, g0, *unused):
        return (None,) + tuple(g * g0 for g in ctx.saved_tensors)


def head_cls_loss(preds, col0, num_class, labels, soft, scale):
    """(loss, #positives) of WeightedClassificationLoss with soft one-hot targets over the rows of preds (n, cols); the class
    logits are columns col0 .. col0 + num_class - 1.  Differentiable wrt preds."""
    p2 = preds.reshape(-1, preds.shape[-1])
    p2 = p2 if p2.is_contiguous() else p2.contiguous()
    n, cols = p2.shape

    def run():
        out = torch.empty((2,), dtype=torch.float32, device=p2.device)
        grad = torch.empty_like(p2)
        _call("pda_head_cls_loss", p2, _chk(p2.detach(), "preds", F32), cols, int(col0), int(num_class), _chk(labels, "labels", I64),
              None if soft is None else _chk(soft, "soft", F32), n, float(scale), _chk(out, "out", F32), _chk(grad, "grad", F32))
        return (out[0], out[1]), (grad.view(preds.shape),)
    return _ScaledGrad.apply(run, preds)


def head_box_loss(preds, labels, cls_labels, code_weights, beta, bins, dir_weight, box_weight):
    """(total, xyzwhl, ori_bin * dir_weight, ori_res) of get_center_box_binori_layer_loss; differentiable wrt preds (n, 6 + 2 bins)."""
    p2 = preds if preds.is_contiguous() else preds.contiguous()
    n = p2.shape[0]

    def run():
        out = torch.empty((4,), dtype=torch.float32, device=p2.device)
        grad = torch.empty_like(p2)
        _call("pda_head_box_loss", p2, _chk(p2.detach(), "preds", F32), _chk(labels, "labels", F32), _chk(cls_labels, "cls_labels", I64),
              None if code_weights is None else _chk(code_weights, "code_weights", F32), float(beta), int(bins), float(dir_weight),
              float(box_weight), n, _chk(out, "out", F32), _chk(grad, "grad", F32))
        return (out[0], out[1], out[2], out[3]), (grad,)
    return _ScaledGrad.apply(run, preds)


def head_vote_loss(mode, origin, offsets, key, gt, batch_size, boxes, num_class, weight):
    """The vote loss (mode 0: LOSS_VOTE_TYPE none, mode 1: ver2); differentiable wrt offsets (n, 4) [bs, dx, dy, dz]."""
    o2 = offsets if offsets.is_contiguous() else offsets.contiguous()
    n = o2.shape[0]

    def run():
        out = torch.empty((1,), dtype=torch.float32, device=o2.device)
        grad = torch.empty_like(o2)
        _call("pda_head_vote_loss", o2, int(mode), _chk(origin, "origin", F32), _chk(o2.detach(), "offsets", F32), _chk(key, "key", I64),
              _chk(gt, "gt", F32), int(batch_size), int(boxes), int(num_class), float(weight), n, _chk(out, "out", F32), _chk(grad, "grad", F32))
        return (out[0],), (grad,)
    return _ScaledGrad.apply(run, offsets)[0]


def head_corner_loss(box_preds, centers, cls_preds, gt, cls_labels, mean_size, bins, weight):
    """get_corner_layer_loss incl. the box decode; differentiable wrt box_preds (n, 6 + 2 bins) and centers (n, 4)."""
    b2 = box_preds if box_preds.is_contiguous() else box_preds.contiguous()
    c2 = centers if centers.is_contiguous() else centers.contiguous()
    k2 = cls_preds.detach().reshape(b2.shape[0], -1).contiguous()
    n = b2.shape[0]

    def run():
        out = torch.empty((1,), dtype=torch.float32, device=b2.device)
        gb, gc = torch.empty_like(b2), torch.empty_like(c2)
        _call("pda_head_corner_loss", b2, _chk(b2.detach(), "box_preds", F32), _chk(c2.detach(), "centers", F32), _chk(k2, "cls_preds", F32),
              int(k2.shape[1]), _chk(gt, "gt", F32), _chk(cls_labels, "cls_labels", I64),
              None if mean_size is None else _chk(mean_size, "mean_size", F32), int(bins), float(weight), n, _chk(out, "out", F32),
              _chk(gb, "grad_box", F32), _chk(gc, "grad_centers", F32))
        return (out[0],), (gb, gc)
    return _ScaledGrad.apply(run, box_preds, centers)[0]


# ---- RoI-aware pooling of the Part-A2 head (roiaware_pool3d_utils.py:9-107; csrc/roi_pool.hip) ---------------------------------
def points_in_boxes_cpu(points, boxes):
    """
    Args:
        points: (num_points, 3)
        boxes: [x, y, z, dx, dy, dz, heading], (x, y, z) is the box center, each box DO NOT overlaps
    Returns:
        point_indices: (N, num_points)
    The reference computes this on the host; here numpy input (or a CPU tensor) travels to the current device and the
    result comes back as numpy (or to the input's device).  The test is the host statement: margin 1e-2, no FMA.
    """
    import numpy as np
    assert boxes.shape[1] == 7
    assert points.shape[1] == 3
    is_numpy = isinstance(points, np.ndarray)
    points = torch.from_numpy(points).float() if is_numpy else points
    boxes = torch.from_numpy(boxes).float() if isinstance(boxes, np.ndarray) else boxes
    home = points.device
    dev = home if home.type == "cuda" else (boxes.device if boxes.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    point_indices = torch.zeros((boxes.shape[0], points.shape[0]), dtype=torch.int, device=dev)
    roiaware_pool3d_cuda.points_in_boxes_cpu(boxes.to(dev).float().contiguous(), points.to(dev).float().contiguous(), point_indices)
    return point_indices.cpu().numpy() if is_numpy else point_indices.to(home)


class RoIAwarePool3d(torch.nn.Module):
    def __init__(self, out_size, max_pts_each_voxel=128):
        super().__init__()
        self.out_size = out_size
        self.max_pts_each_voxel = max_pts_each_voxel

    def forward(self, rois, pts, pts_feature, pool_method='max'):
        assert pool_method in ['max', 'avg']
        return RoIAwarePool3dFunction.apply(rois, pts, pts_feature, self.out_size, self.max_pts_each_voxel, pool_method)


class RoIAwarePool3dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rois, pts, pts_feature, out_size, max_pts_each_voxel, pool_method):
        """
        Args:
            rois: (N, 7) [x, y, z, dx, dy, dz, heading] (x, y, z) is the box center
            pts: (npoints, 3)
            pts_feature: (npoints, C)
            out_size: int or tuple, like 7 or (7, 7, 7)
            max_pts_each_voxel:
            pool_method: 'max' or 'avg'
        Returns:
            pooled_features: (N, out_x, out_y, out_z, C)
        """
        assert rois.shape[1] == 7 and pts.shape[1] == 3
        if isinstance(out_size, int):
            out_x = out_y = out_z = out_size
        else:
            assert len(out_size) == 3
            for k in range(3):
                assert isinstance(out_size[k], int)
            out_x, out_y, out_z = out_size
        num_rois, num_channels, num_pts = rois.shape[0], pts_feature.shape[-1], pts.shape[0]
        pooled_features = pts_feature.new_zeros((num_rois, out_x, out_y, out_z, num_channels))
        argmax = pts_feature.new_zeros((num_rois, out_x, out_y, out_z, num_channels), dtype=torch.int)
        pts_idx_of_voxels = pts_feature.new_zeros((num_rois, out_x, out_y, out_z, max_pts_each_voxel), dtype=torch.int)
        pool_method = {'max': 0, 'avg': 1}[pool_method]
        roiaware_pool3d_cuda.forward(rois.contiguous(), pts.contiguous(), pts_feature.contiguous(), argmax, pts_idx_of_voxels,
                                     pooled_features, pool_method)
        ctx.roiaware_pool3d_for_backward = (pts_idx_of_voxels, argmax, pool_method, num_pts, num_channels)
        return pooled_features

    @staticmethod
    def backward(ctx, grad_out):
        """grad_out (N, out_x, out_y, out_z, C) -> grad_in (npoints, C) for pts_feature, None for the other inputs"""
        pts_idx_of_voxels, argmax, pool_method, num_pts, num_channels = ctx.roiaware_pool3d_for_backward
        grad_in = grad_out.new_zeros((num_pts, num_channels))
        roiaware_pool3d_cuda.backward(pts_idx_of_voxels, argmax, grad_out.contiguous(), grad_in, pool_method)
        return None, None, grad_in, None, None, None
