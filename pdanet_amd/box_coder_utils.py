"""Box coders.  `ResidualCoder` (pcdet/utils/box_coder_utils.py:5-77) is the coder of the two-stage RoI heads
(roi_head_template.py): residuals against an anchor box, scaled by the anchor's BEV diagonal and height, log size ratios and
a heading difference (or cos / sin differences).

Box coder of both PDA-SSD yamls (`PointResidual_BinOri_Coder`, pcdet/utils/box_coder_utils.py:224-319): a box is coded
against the point that predicts it as

    [ (centre - point) / (d, d, h) | log(size / (l, w, h)) | heading bin | heading residual in [-1, 1] | extras ]

with (l, w, h) the mean size of the box's class and d = sqrt(l^2 + w^2) (or, without mean sizes, plain differences and
log sizes).  The heading is one of `bin_size` equal sectors of [-pi, pi) plus the offset from the sector's middle in
units of half a sector.  Written on (N, 3) blocks; element for element the reference's arithmetic (the head's golden
tensors pin it, tests/test_iassd_head.py).  On the GPU the training path never decodes (csrc/head_loss.hip carries the
decode inside the corner loss); this module is the eval decode and the reference formulation the kernels are checked against."""
import math

import torch


class PointResidual_BinOri_Coder(object):  # noqa: N801 (the yaml names the class)
    def __init__(self, code_size=8, use_mean_size=True, **kwargs):
        self.bin_size = kwargs.get('bin_size', 12)       # (the yaml's 'angle_bin_num' key is not read by the reference, :227)
        self.code_size = 6 + 2 * self.bin_size
        self.bin_inter = 2 * math.pi / self.bin_size
        self.use_mean_size = use_mean_size
        self.mean_size = None
        if use_mean_size:
            self.mean_size = torch.tensor(kwargs['mean_size'], dtype=torch.float32)
            assert self.mean_size.min() > 0

    def _mean(self, like):
        """The (num_class, 3) mean sizes on `like`'s device (the reference moves them to the GPU at construction, :234)."""
        if self.mean_size.device != like.device:
            self.mean_size = self.mean_size.to(like.device)
        return self.mean_size

    def _scales(self, classes, like):
        """Per-row divisors of the centre residual (d, d, h) and of the size ratio (l, w, h), or None without mean sizes."""
        if not self.use_mean_size:
            return None, None
        anchor = self._mean(like)[classes - 1]                                  # classes are 1-based
        diag = torch.sqrt(anchor[..., 0:1] ** 2 + anchor[..., 1:2] ** 2)
        return torch.cat([diag, diag, anchor[..., 2:3]], dim=-1), anchor

    def encode_torch(self, gt_boxes, points, gt_classes=None):
        """(N, 7 + C) boxes, (N, 3) points, (N) classes in [1, num_class] -> (N, 8 + C) codes."""
        size = torch.clamp_min(gt_boxes[:, 3:6], min=1e-5)
        ctr_div, anchor = self._scales(gt_classes, gt_boxes)
        offset = gt_boxes[:, 0:3] - points
        if anchor is not None:
            offset, size = offset / ctr_div, size / anchor
        heading = torch.clamp(gt_boxes[:, 6:7], max=math.pi - 1e-5, min=-math.pi + 1e-5) + math.pi     # in (0, 2 pi)
        sector = torch.floor(heading / self.bin_inter)
        within = (heading - (sector * self.bin_inter + self.bin_inter / 2)) / (self.bin_inter / 2)
        return torch.cat([offset, torch.log(size), sector, within, gt_boxes[:, 7:]], dim=-1)

    def decode_torch(self, box_encodings, points, pred_classes=None):
        """(N, 6 + 2 bin_size) codes, (N, 3) points -> (N, 7) boxes; the heading bin is the arg-max of the bin scores."""
        nb = self.bin_size
        ctr_div, anchor = self._scales(pred_classes, box_encodings)
        centre, size = box_encodings[..., 0:3], torch.exp(box_encodings[..., 3:6])
        if anchor is not None:
            centre, size = centre * ctr_div, size * anchor
        centre = centre + points
        sector = torch.argmax(box_encodings[..., 6:6 + nb], dim=-1, keepdim=True)
        within = torch.gather(box_encodings[..., 6 + nb:6 + 2 * nb], -1, sector)
        heading = sector.float() * self.bin_inter - math.pi + self.bin_inter / 2
        return torch.cat([centre, size, heading + within * (self.bin_inter / 2)], dim=-1)


class PointResidualCoder(object):
    """pcdet/utils/box_coder_utils.py:144-221, the coder of PointHeadBox: a box against the point that predicts it as
    [(centre - point) / (d, d, h) | log(size / (l, w, h)) | cos heading | sin heading | extras], (l, w, h) the mean size of
    the class and d = sqrt(l^2 + w^2); without mean sizes plain differences and log sizes."""

    def __init__(self, code_size=8, use_mean_size=True, **kwargs):
        self.code_size = code_size
        self.use_mean_size = use_mean_size
        self.mean_size = None
        if use_mean_size:
            self.mean_size = torch.tensor(kwargs['mean_size'], dtype=torch.float32)
            assert self.mean_size.min() > 0

    def _anchor(self, classes, like):
        """The (N, 3) mean sizes of the 1-based classes, in `like`'s device and type."""
        if self.mean_size.device != like.device:
            self.mean_size = self.mean_size.to(like.device)
        return self.mean_size.to(like.dtype)[classes - 1]

    def encode_torch(self, gt_boxes, points, gt_classes=None):
        """(N, 7 + C) boxes, (N, 3) points, (N) classes in [1, num_class] -> (N, 8 + C) codes.  The sizes are clamped to 1e-5 on
        a copy: unlike the reference's (:162) this encode leaves its argument untouched."""
        xg, yg, zg, dxg, dyg, dzg, rg, *cgs = torch.split(gt_boxes, 1, dim=-1)
        dxg, dyg, dzg = (torch.clamp_min(v, min=1e-5) for v in (dxg, dyg, dzg))
        xa, ya, za = torch.split(points, 1, dim=-1)
        if self.use_mean_size:
            dxa, dya, dza = torch.split(self._anchor(gt_classes, gt_boxes), 1, dim=-1)
            diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
            xt, yt, zt = (xg - xa) / diagonal, (yg - ya) / diagonal, (zg - za) / dza
            dxt, dyt, dzt = torch.log(dxg / dxa), torch.log(dyg / dya), torch.log(dzg / dza)
        else:
            xt, yt, zt = xg - xa, yg - ya, zg - za
            dxt, dyt, dzt = torch.log(dxg), torch.log(dyg), torch.log(dzg)
        return torch.cat([xt, yt, zt, dxt, dyt, dzt, torch.cos(rg), torch.sin(rg), *cgs], dim=-1)

    def decode_torch(self, box_encodings, points, pred_classes=None):
        """(N, 8 + C) codes, (N, 3) points, (N) classes in [1, num_class] -> (N, 7 + C) boxes."""
        xt, yt, zt, dxt, dyt, dzt, cost, sint, *cts = torch.split(box_encodings, 1, dim=-1)
        xa, ya, za = torch.split(points, 1, dim=-1)
        if self.use_mean_size:
            dxa, dya, dza = torch.split(self._anchor(pred_classes, box_encodings), 1, dim=-1)
            diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
            xg, yg, zg = xt * diagonal + xa, yt * diagonal + ya, zt * dza + za
            dxg, dyg, dzg = torch.exp(dxt) * dxa, torch.exp(dyt) * dya, torch.exp(dzt) * dza
        else:
            xg, yg, zg = xt + xa, yt + ya, zt + za
            dxg, dyg, dzg = torch.exp(dxt), torch.exp(dyt), torch.exp(dzt)
        rg = torch.atan2(sint, cost)
        return torch.cat([xg, yg, zg, dxg, dyg, dzg, rg, *cts], dim=-1)


class ResidualCoder(object):
    def __init__(self, code_size=7, encode_angle_by_sincos=False, **kwargs):
        self.code_size = code_size
        self.encode_angle_by_sincos = encode_angle_by_sincos
        if self.encode_angle_by_sincos:
            self.code_size += 1

    def encode_torch(self, boxes, anchors):
        """boxes (N, 7 + C), anchors (N, 7 + C) -> (N, 7 + C) codes (8 + C with encode_angle_by_sincos).  Sizes are clamped to
        1e-5 on copies: unlike the reference's (:22-23) this encode leaves its arguments untouched."""
        xa, ya, za, dxa, dya, dza, ra, *cas = torch.split(anchors, 1, dim=-1)
        xg, yg, zg, dxg, dyg, dzg, rg, *cgs = torch.split(boxes, 1, dim=-1)
        dxa, dya, dza = (torch.clamp_min(v, min=1e-5) for v in (dxa, dya, dza))
        dxg, dyg, dzg = (torch.clamp_min(v, min=1e-5) for v in (dxg, dyg, dzg))
        diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
        xt, yt, zt = (xg - xa) / diagonal, (yg - ya) / diagonal, (zg - za) / dza
        dxt, dyt, dzt = torch.log(dxg / dxa), torch.log(dyg / dya), torch.log(dzg / dza)
        if self.encode_angle_by_sincos:
            rts = [torch.cos(rg) - torch.cos(ra), torch.sin(rg) - torch.sin(ra)]
        else:
            rts = [rg - ra]
        cts = [g - a for g, a in zip(cgs, cas)]
        return torch.cat([xt, yt, zt, dxt, dyt, dzt, *rts, *cts], dim=-1)

    def decode_torch(self, box_encodings, anchors):
        """box_encodings (B, N, 7 + C) or (N, 7 + C) codes, anchors of the same leading shape -> boxes."""
        xa, ya, za, dxa, dya, dza, ra, *cas = torch.split(anchors, 1, dim=-1)
        if not self.encode_angle_by_sincos:
            xt, yt, zt, dxt, dyt, dzt, rt, *cts = torch.split(box_encodings, 1, dim=-1)
        else:
            xt, yt, zt, dxt, dyt, dzt, cost, sint, *cts = torch.split(box_encodings, 1, dim=-1)
        diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
        xg, yg, zg = xt * diagonal + xa, yt * diagonal + ya, zt * dza + za
        dxg, dyg, dzg = torch.exp(dxt) * dxa, torch.exp(dyt) * dya, torch.exp(dzt) * dza
        if self.encode_angle_by_sincos:
            rg = torch.atan2(sint + torch.sin(ra), cost + torch.cos(ra))
        else:
            rg = rt + ra
        cgs = [t + a for t, a in zip(cts, cas)]
        return torch.cat([xg, yg, zg, dxg, dyg, dzg, rg, *cgs], dim=-1)
