"""ImageVFE (pcdet/models/backbones_3d/vfe/image_vfe.py) with what it is built of: DepthFFN, FrustumToVoxel, DDNLoss and
BasicBlock2D, under the reference's names, constructor arguments, config keys and state-dict keys (children ffn, f2v; ffn.ddn,
ffn.channel_reduce).

The reference's DepthFFN forms frustum_features = softmax(depth_logits)[:, :-1] x image_features (B, C, D, Hf, Wf) and
FrustumToVoxel samples it with a (B, X, Y, Z, 3) grid through a 5-D grid_sample.  Here DepthFFN leaves the two factors in the
batch (`image_features`, `depth_logits`) and FrustumToVoxel, for `mode: bilinear` with `padding_mode: zeros`, calls
`frustum_sample` (csrc/frustum_sample.hip): neither the frustum tensor, nor its gradient, nor the grid exists; the arithmetic
is stated in include/pda_train.h.  PDA_FRUSTUM_SAMPLE=composed keeps the reference's torch composition
(`frustum_to_voxel_composed`), which also serves every other sampler setting, runs on CPU tensors and in float64, and is the
tests' yardstick.  No kornia: the voxel grid is (i + 0.5, j + 0.5, k + 0.5), points become homogeneous by a 1, and
convert_points_from_homogeneous multiplies by 1 / z where |z| > 1e-8 and by 1 elsewhere.

DDNLoss is one pass on the device (pda_ddn_loss_fwd_bwd): loss and d logits together, no host read, gt_boxes2d left as it
is (the reference's compute_fg_mask divides the caller's boxes in place).  PDA_DDN_LOSS=composed selects `ddn_loss_composed`,
the same formula in torch.  tb_dict values are 0-dim device tensors.

Out of scope: the image-side data steps (random_image_flip, calculate_grid_size, downsample_depth_map), aux_loss."""
import ctypes
import math
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from .config import fused_or_composed
from .ddn_deeplabv3 import DDNDeepLabV3
from .pointnet2_batch_cuda import F32, _call, _chk

ENV = "PDA_FRUSTUM_SAMPLE"
ENV_LOSS = "PDA_DDN_LOSS"
sample_path = partial(fused_or_composed, ENV)
loss_path = partial(fused_or_composed, ENV_LOSS)
MODES = {'UD': 0, 'LID': 1, 'SID': 2}
OUT_OF_BOUNDS = -2


class BasicBlock2D(nn.Module):
    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.conv = nn.Conv2d(in_channels=in_channels, out_channels=out_channels, **kwargs)
        self.bn = nn.BatchNorm2d(out_channels)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, features):
        return self.relu(self.bn(self.conv(features)))


def bin_depths(depth_map, mode, depth_min, depth_max, num_bins, target=False):
    """transform_utils.bin_depths: the continuous bin index; target=True: outside [0, num_bins] or not finite -> num_bins, int64."""
    if mode == "UD":
        indices = (depth_map - depth_min) / ((depth_max - depth_min) / num_bins)
    elif mode == "LID":
        bin_size = 2 * (depth_max - depth_min) / (num_bins * (1 + num_bins))
        indices = -0.5 + 0.5 * torch.sqrt(1 + 8 * (depth_map - depth_min) / bin_size)
    elif mode == "SID":
        indices = num_bins * (torch.log(1 + depth_map) - math.log(1 + depth_min)) / \
            (math.log(1 + depth_max) - math.log(1 + depth_min))
    else:
        raise NotImplementedError("DISCRETIZE.mode %r (UD, LID, SID)" % (mode,))
    if target:
        mask = (indices < 0) | (indices > num_bins) | (~torch.isfinite(indices))
        indices = torch.where(mask, torch.full_like(indices, num_bins), indices).type(torch.int64)
    return indices


def voxel_geometry32(grid_size, pc_range):
    """(pc_min, voxel_size) as lists of Python floats holding the float32 values the reference's generator computes."""
    pc = torch.as_tensor([float(v) for v in pc_range], dtype=torch.float32).reshape(2, 3)
    size = (pc[1] - pc[0]) / torch.as_tensor([float(v) for v in grid_size], dtype=torch.float32)
    return pc[0].tolist(), size.tolist()


def create_frustum_features(image_features, depth_logits):
    """DepthFFN.create_frustum_features: (N, C, H, W), (N, D + 1, H, W) -> (N, C, D, H, W)."""
    depth_probs = F.softmax(depth_logits.unsqueeze(1), dim=2)[:, :, :-1]
    return depth_probs * image_features.unsqueeze(2)


def frustum_grid(lidar_to_cam, cam_to_img, image_shape, grid_size, pc_range, disc_cfg):
    """FrustumGridGenerator.forward: the normalised (B, X, Y, Z, 3) sampling grid, in the dtype of lidar_to_cam."""
    dtype, dev = lidar_to_cam.dtype, lidar_to_cam.device
    B = lidar_to_cam.shape[0]
    X, Y, Z = (int(v) for v in grid_size)
    pc_min, size = voxel_geometry32(grid_size, pc_range)
    ar = [torch.arange(n, dtype=dtype, device=dev) for n in (X, Y, Z)]
    voxel_grid = torch.stack(torch.meshgrid(*ar, indexing='ij'), dim=-1) + 0.5                      # (X, Y, Z, 3)
    unproject = torch.tensor([[size[0], 0, 0, pc_min[0]], [0, size[1], 0, pc_min[1]], [0, 0, size[2], pc_min[2]],
                              [0, 0, 0, 1]], dtype=dtype, device=dev)
    trans = (lidar_to_cam @ unproject).reshape(B, 1, 1, 1, 4, 4)
    ones = torch.ones((B, X, Y, Z, 1), dtype=dtype, device=dev)
    points = torch.cat((voxel_grid.unsqueeze(0).expand(B, X, Y, Z, 3), ones), dim=-1).unsqueeze(-1)
    camera = (trans @ points)[..., :3, :]
    project = cam_to_img.reshape(B, 1, 1, 1, 3, 4)
    points_t = (project @ torch.cat((camera, ones.unsqueeze(-1)), dim=-2)).squeeze(-1)              # (B, X, Y, Z, 3)
    z = points_t[..., -1:]
    scale = torch.where(torch.abs(z) > 1e-8, 1.0 / z, torch.ones_like(z))
    image_grid = scale * points_t[..., :-1]
    depths = bin_depths(points_t[..., -1] - project[..., 2, 3], **disc_cfg)
    grid = torch.cat((image_grid, depths.unsqueeze(-1)), dim=-1)
    hw = torch.max(image_shape, dim=0)[0].to(device=dev)
    shape = torch.cat((hw.flip(0), torch.tensor([disc_cfg["num_bins"]], device=dev, dtype=hw.dtype)))   # (W, H, D)
    grid = grid / (shape - 1) * 2 + -1
    return torch.where(torch.isfinite(grid), grid, torch.full_like(grid, OUT_OF_BOUNDS))


def frustum_to_voxel_composed(image_features, depth_logits, lidar_to_cam, cam_to_img, image_shape, grid_size, pc_range,
                              disc_cfg, mode="bilinear", padding_mode="zeros"):
    """The reference's composition: frustum features, the grid, F.grid_sample, the permute to (B, C, Z, Y, X)."""
    frustum = create_frustum_features(image_features, depth_logits)
    grid = frustum_grid(lidar_to_cam.to(frustum.dtype), cam_to_img.to(frustum.dtype), image_shape, grid_size, pc_range, disc_cfg)
    out = F.grid_sample(input=frustum, grid=grid, mode=mode, padding_mode=padding_mode, align_corners=False)
    return out.permute(0, 1, 4, 3, 2)


def _geometry_args(feat, prob, grid_size, pc_range, disc_cfg):
    B, C, Hf, Wf = (int(v) for v in feat.shape)
    D = int(prob.shape[1])
    pc_min, size = voxel_geometry32(grid_size, pc_range)
    f3 = ctypes.c_float * 3
    X, Y, Z = (int(v) for v in grid_size)
    return (B, C, D, Hf, Wf, X, Y, Z, f3(*pc_min), f3(*size), MODES[disc_cfg["mode"]], float(disc_cfg["depth_min"]),
            float(disc_cfg["depth_max"]))


class _FrustumSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, prob, lidar_to_cam, cam_to_img, image_hw, grid_size, pc_range, disc_cfg):
        feat, prob = feat.contiguous(), prob.contiguous()
        args = _geometry_args(feat, prob, grid_size, pc_range, disc_cfg)
        B, C = args[0], args[1]
        X, Y, Z = args[5:8]
        out = torch.empty((B, C, Z, Y, X), dtype=F32, device=feat.device)
        _call("pda_frustum_sample_fwd", feat, _chk(feat, "image_features", F32), _chk(prob, "depth_probs", F32),
              _chk(lidar_to_cam, "trans_lidar_to_cam", F32), _chk(cam_to_img, "trans_cam_to_img", F32),
              _chk(image_hw, "image_hw", F32), out.data_ptr(), *args)
        ctx.save_for_backward(feat, prob, lidar_to_cam, cam_to_img, image_hw)
        ctx.args = args
        return out

    @staticmethod
    def backward(ctx, grad_out):
        feat, prob, lidar_to_cam, cam_to_img, image_hw = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        grad_feat, grad_prob = torch.zeros_like(feat), torch.zeros_like(prob)
        _call("pda_frustum_sample_bwd", feat, _chk(grad_out, "grad_out", F32), feat.data_ptr(), prob.data_ptr(),
              lidar_to_cam.data_ptr(), cam_to_img.data_ptr(), image_hw.data_ptr(), grad_feat.data_ptr(), grad_prob.data_ptr(),
              *ctx.args)
        return grad_feat, grad_prob, None, None, None, None, None, None


def frustum_sample(image_features, depth_probs, lidar_to_cam, cam_to_img, image_shape, grid_size, pc_range, disc_cfg):
    """image_features (B, C, Hf, Wf), depth_probs (B, D, Hf, Wf) = softmax(depth_logits)[:, :-1], lidar_to_cam (B, 4, 4),
    cam_to_img (B, 3, 4), image_shape (B, 2) [H, W] -> voxel_features (B, C, Z, Y, X), with gradients to the first two.
    One launch each way; the batch maximum of image_shape is taken on the device."""
    if image_features.dim() != 4 or depth_probs.dim() != 4 or depth_probs.shape[0] != image_features.shape[0] \
            or depth_probs.shape[2:] != image_features.shape[2:] or int(depth_probs.shape[1]) != int(disc_cfg["num_bins"]):
        raise ValueError("image_features must be (B, C, Hf, Wf) and depth_probs (B, num_bins, Hf, Wf), got %s and %s"
                         % (tuple(image_features.shape), tuple(depth_probs.shape)))
    B = image_features.shape[0]
    if tuple(lidar_to_cam.shape) != (B, 4, 4) or tuple(cam_to_img.shape) != (B, 3, 4) or tuple(image_shape.shape) != (B, 2):
        raise ValueError("lidar_to_cam must be (B, 4, 4), cam_to_img (B, 3, 4) and image_shape (B, 2), got %s, %s and %s"
                         % (tuple(lidar_to_cam.shape), tuple(cam_to_img.shape), tuple(image_shape.shape)))
    dev = image_features.device
    image_hw = torch.max(image_shape.to(dev), dim=0)[0].to(F32).contiguous()
    return _FrustumSample.apply(image_features, depth_probs, lidar_to_cam.to(device=dev, dtype=F32).contiguous(),
                                cam_to_img.to(device=dev, dtype=F32).contiguous(), image_hw, grid_size, pc_range, disc_cfg)


class FrustumToVoxel(nn.Module):
    def __init__(self, model_cfg, grid_size, pc_range, disc_cfg):
        super().__init__()
        self.model_cfg = model_cfg
        self.grid_size = [int(v) for v in grid_size]
        self.pc_range = [float(v) for v in pc_range]
        self.disc_cfg = dict(disc_cfg)
        if self.disc_cfg["mode"] not in MODES:
            raise NotImplementedError("DISCRETIZE.mode %r (UD, LID, SID)" % (self.disc_cfg["mode"],))
        sampler = dict(model_cfg['SAMPLER'])
        self.mode, self.padding_mode = sampler.get("mode", "bilinear"), sampler.get("padding_mode", "zeros")

    def forward(self, batch_dict):
        """image_features (B, C, Hf, Wf), depth_logits (B, D + 1, Hf, Wf), trans_lidar_to_cam, trans_cam_to_img, image_shape
        -> voxel_features (B, C, Z, Y, X)."""
        feat, logits = batch_dict["image_features"], batch_dict["depth_logits"]
        geo = (batch_dict["trans_lidar_to_cam"], batch_dict["trans_cam_to_img"], batch_dict["image_shape"], self.grid_size,
               self.pc_range, self.disc_cfg)
        if sample_path() == "fused" and (self.mode, self.padding_mode) == ("bilinear", "zeros"):
            probs = F.softmax(logits, dim=1)[:, :-1]
            batch_dict["voxel_features"] = frustum_sample(feat, probs, *geo)
        else:
            batch_dict["voxel_features"] = frustum_to_voxel_composed(feat, logits, *geo, mode=self.mode,
                                                                     padding_mode=self.padding_mode)
        return batch_dict


# ---- DDNLoss ------------------------------------------------------------------------------------------------------------------
def fg_mask(gt_boxes2d, shape, downsample_factor):
    """loss_utils.compute_fg_mask without its in-place division: (B, H, W) bool, a pixel (v, u) is foreground if it lies in any
    [floor(u1 / f), ceil(u2 / f)) x [floor(v1 / f), ceil(v2 / f))."""
    B, H, W = shape
    boxes = gt_boxes2d / downsample_factor
    u1, v1 = torch.floor(boxes[..., 0]), torch.floor(boxes[..., 1])
    u2, v2 = torch.ceil(boxes[..., 2]), torch.ceil(boxes[..., 3])
    u = torch.arange(W, device=boxes.device, dtype=boxes.dtype).view(1, 1, 1, W)
    v = torch.arange(H, device=boxes.device, dtype=boxes.dtype).view(1, 1, H, 1)
    inside = (u >= u1[..., None, None]) & (u < u2[..., None, None]) & (v >= v1[..., None, None]) & (v < v2[..., None, None])
    return inside.any(dim=1)


def ddn_loss_composed(depth_logits, depth_maps, gt_boxes2d, disc_cfg, downsample_factor, weight, alpha, gamma, fg_weight,
                      bg_weight):
    """(loss, fg_loss, bg_loss) in torch, in the dtype of depth_logits: the focal term -alpha (1 - p_t)^gamma log_softmax(x)_t,
    the foreground / background weights, sums over the pixels divided by their number."""
    target = bin_depths(depth_maps.to(depth_logits.dtype), **disc_cfg, target=True)
    logp = F.log_softmax(depth_logits, dim=1).gather(1, target.unsqueeze(1)).squeeze(1)
    p = F.softmax(depth_logits, dim=1).gather(1, target.unsqueeze(1)).squeeze(1)
    loss = -alpha * torch.pow(1.0 - p, gamma) * logp
    fg = fg_mask(gt_boxes2d.to(depth_logits.dtype), loss.shape, downsample_factor)
    loss = loss * (fg_weight * fg + bg_weight * (~fg)).to(loss.dtype)
    pixels = fg.numel()
    fg_loss, bg_loss = loss[fg].sum() / pixels, loss[~fg].sum() / pixels
    return (fg_loss + bg_loss) * weight, fg_loss, bg_loss


class _DDNLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, depth_maps, boxes, host):
        from . import _lib
        mode, depth_min, depth_max, downsample, alpha, gamma, fg_weight, bg_weight, weight = host
        logits, depth_maps, boxes = logits.contiguous(), depth_maps.contiguous(), boxes.contiguous()
        B, D1, H, W = (int(v) for v in logits.shape)
        grad = torch.empty_like(logits)
        out3 = torch.empty((3,), dtype=F32, device=logits.device)
        partials = torch.empty((2 * int(_lib.load().pda_ddn_loss_blocks(B * H * W)),), dtype=torch.float64, device=logits.device)
        _call("pda_ddn_loss_fwd_bwd", logits, _chk(logits, "depth_logits", F32), _chk(depth_maps, "depth_maps", F32),
              _chk(boxes, "gt_boxes2d", F32) if boxes.numel() else None, grad.data_ptr(), partials.data_ptr(), out3.data_ptr(),
              B, D1 - 1, H, W, int(boxes.shape[1]), mode, depth_min, depth_max, downsample, alpha, gamma, fg_weight, bg_weight,
              weight)
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(out3)
        return out3[0].clone(), out3

    @staticmethod
    def backward(ctx, grad_loss, _):
        grad, = ctx.saved_tensors
        return grad * grad_loss, None, None, None


class DDNLoss(nn.Module):
    def __init__(self, weight, alpha, gamma, disc_cfg, fg_weight, bg_weight, downsample_factor):
        super().__init__()
        self.disc_cfg = dict(disc_cfg)
        if self.disc_cfg["mode"] not in MODES:
            raise NotImplementedError("DISCRETIZE.mode %r (UD, LID, SID)" % (self.disc_cfg["mode"],))
        self.weight, self.alpha, self.gamma = float(weight), float(alpha), float(gamma)
        self.fg_weight, self.bg_weight, self.downsample_factor = float(fg_weight), float(bg_weight), float(downsample_factor)

    def forward(self, depth_logits, depth_maps, gt_boxes2d):
        """depth_logits (B, D + 1, H, W), depth_maps (B, H, W) in metres (NaN where padded), gt_boxes2d (B, N, 4) zero-padded
        -> (loss, tb_dict); gt_boxes2d is not written."""
        B, D1, H, W = depth_logits.shape
        if D1 != self.disc_cfg["num_bins"] + 1 or tuple(depth_maps.shape) != (B, H, W) or gt_boxes2d.dim() != 3 \
                or gt_boxes2d.shape[0] != B or gt_boxes2d.shape[2] != 4:
            raise ValueError("depth_logits must be (B, num_bins + 1, H, W), depth_maps (B, H, W) and gt_boxes2d (B, N, 4), got "
                             "%s, %s and %s" % (tuple(depth_logits.shape), tuple(depth_maps.shape), tuple(gt_boxes2d.shape)))
        if loss_path() == "fused":
            host = (MODES[self.disc_cfg["mode"]], float(self.disc_cfg["depth_min"]), float(self.disc_cfg["depth_max"]),
                    self.downsample_factor, self.alpha, self.gamma, self.fg_weight, self.bg_weight, self.weight)
            loss, out3 = _DDNLoss.apply(depth_logits, depth_maps.to(F32), gt_boxes2d.to(F32), host)
            fg_loss, bg_loss = out3[1], out3[2]
        else:
            loss, fg_loss, bg_loss = ddn_loss_composed(depth_logits, depth_maps, gt_boxes2d, self.disc_cfg, self.downsample_factor,
                                                       self.weight, self.alpha, self.gamma, self.fg_weight, self.bg_weight)
        tb_dict = {"balancer_loss": (fg_loss + bg_loss).detach(), "fg_loss": fg_loss.detach(), "bg_loss": bg_loss.detach(),
                   "ddn_loss": loss.detach()}
        return loss, tb_dict


# ---- DepthFFN, ImageVFE ---------------------------------------------------------------------------------------------------------
class DepthFFN(nn.Module):
    DDN = {'DDNDeepLabV3': DDNDeepLabV3}
    LOSS = {'DDNLoss': DDNLoss}

    def __init__(self, model_cfg, downsample_factor):
        super().__init__()
        self.model_cfg = model_cfg
        self.disc_cfg = dict(model_cfg['DISCRETIZE'])
        self.downsample_factor = downsample_factor
        for key, table in (('DDN', self.DDN), ('LOSS', self.LOSS)):
            if model_cfg[key]['NAME'] not in table:
                raise NotImplementedError("FFN.%s.NAME %r (%s)" % (key, model_cfg[key]['NAME'], ", ".join(table)))
        ddn_cfg = model_cfg['DDN']
        self.ddn = self.DDN[ddn_cfg['NAME']](num_classes=self.disc_cfg["num_bins"] + 1, backbone_name=ddn_cfg['BACKBONE_NAME'],
                                             **dict(ddn_cfg['ARGS']))
        self.channel_reduce = BasicBlock2D(**dict(model_cfg['CHANNEL_REDUCE']))
        # no parameters and no buffers: the state dict has no ddn_loss keys, as in the reference
        self.ddn_loss = self.LOSS[model_cfg['LOSS']['NAME']](disc_cfg=self.disc_cfg, downsample_factor=downsample_factor,
                                                             **dict(model_cfg['LOSS']['ARGS']))
        self.forward_ret_dict = {}

    def get_output_feature_dim(self):
        return self.channel_reduce.out_channels

    def forward(self, batch_dict):
        """images (N, 3, H, W) -> image_features (N, C, Hf, Wf) and depth_logits (N, D + 1, Hf, Wf): the two factors of the
        reference's frustum_features."""
        ddn_result = self.ddn(batch_dict["images"])
        depth_logits = ddn_result["logits"]
        batch_dict["image_features"] = self.channel_reduce(ddn_result["features"])
        batch_dict["depth_logits"] = depth_logits
        if self.training:
            self.forward_ret_dict["depth_maps"] = batch_dict["depth_maps"]
            self.forward_ret_dict["gt_boxes2d"] = batch_dict["gt_boxes2d"]
            self.forward_ret_dict["depth_logits"] = depth_logits
        return batch_dict

    def get_loss(self):
        return self.ddn_loss(**self.forward_ret_dict)


class ImageVFE(nn.Module):
    FFN = {'DepthFFN': DepthFFN}
    F2V = {'FrustumToVoxel': FrustumToVoxel}

    def __init__(self, model_cfg, grid_size, point_cloud_range, depth_downsample_factor, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.grid_size, self.pc_range, self.downsample_factor = grid_size, point_cloud_range, depth_downsample_factor
        for key, table in (('FFN', self.FFN), ('F2V', self.F2V)):
            if model_cfg[key]['NAME'] not in table:
                raise NotImplementedError("VFE.%s.NAME %r (%s)" % (key, model_cfg[key]['NAME'], ", ".join(table)))
        self.ffn = self.FFN[model_cfg['FFN']['NAME']](model_cfg=model_cfg['FFN'], downsample_factor=depth_downsample_factor)
        self.disc_cfg = self.ffn.disc_cfg
        self.f2v = self.F2V[model_cfg['F2V']['NAME']](model_cfg=model_cfg['F2V'], grid_size=grid_size, pc_range=point_cloud_range,
                                                      disc_cfg=self.disc_cfg)

    def get_output_feature_dim(self):
        return self.ffn.get_output_feature_dim()

    def forward(self, batch_dict, **kwargs):
        return self.f2v(self.ffn(batch_dict))

    def get_loss(self):
        return self.ffn.get_loss()
