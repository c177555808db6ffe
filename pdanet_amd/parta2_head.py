"""PartA2FCHead (pcdet/models/roi_heads/partA2_head.py), the RoI head of Part-A2: RoI-aware pooling of the point head's part
locations (avg) and of UNetV2's point features (max) into a POOL_SIZE^3 grid per RoI, two sparse-convolution stacks over the
non-empty voxels, and the fc stacks and rcnn losses of RoIHeadTemplate -- under the reference's attribute names (conv_part,
conv_rpn, shared_fc_layer, cls_layers, reg_layers, roiaware_pool3d_layer), so a reference checkpoint loads with strict=True.

The input stage (`parta2_pool`, csrc/parta2.hip).  The reference loops over the scenes with a boolean mask (a host read each),
collects every scene's points into the RoIs' voxels twice -- once for the avg pool, once for the max pool, each with its own
(N, P, P, P, K) int32 table --, builds the masked part features as a tensor, finds the live voxels with nonzero() (another
host read) and gathers their rows from the dense pooled tensors.  Here the scene segments are found on the device, ONE
collection pass serves both poolings, the masking is done in the avg pool's operand read, and the live voxels come out as
sparse rows in nonzero()'s order; the one host read is the live count, by which the worst-case buffers are sliced.
A voxel is live iff the float32 sum of its four pooled part channels, added in channel order, is not zero.

PDA_PARTA2_POOL=composed (read at every forward) selects the reference's order of work on the existing operators instead:
per-scene masks, two RoIAwarePool3d calls, nonzero, indexing.  Both paths give the same bits in the forward.

Fewer than 3 live voxels: the reference's `fake_sparse_idx` -- voxel (0, 0, 0) of every RoI stands in, and in training the
targets are filled with -1 --, decided on the host from the count already read.

Target sampling: batch_dict may carry 'roi_target_seed' or 'roi_target_draws' (ProposalTargetLayer.forward's seed / draws)."""
import torch
import torch.nn as nn

from . import spconv_utils as spconv
from .config import fused_or_composed
from .pointnet2_batch_cuda import F32, I32, _call, _chk
from .roi_head_template import RoIHeadTemplate
from .roiaware_pool3d_utils import RoIAwarePool3d
from .stage_common import workspace

MAX_POOL_SIZE = 16        # csrc/parta2.hip PP_MAX_OUT: the voxel counters of a RoI live in LDS


class _PartA2Pool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, point_features, point_part_offset, rois, point_coords, scores, host):
        thresh, out, k_slots, disable_part, check = host
        dev = point_features.device
        B, N = rois.shape[0], rois.shape[1]
        P, C, total, n_vox = point_coords.shape[0], point_features.shape[1], B * N, out ** 3
        cap = total * n_vox
        seg = torch.empty((B + 1,), dtype=I32, device=dev)
        flag = torch.zeros((1,), dtype=I32, device=dev) if check else None
        table = torch.empty((total, n_vox, k_slots), dtype=I32, device=dev)        # not filled: every count is written
        ws = workspace("pda_parta2_pool_workspace_bytes", (total, out), "%d RoIs of %d^3 voxels are too many" % (total, out), dev)
        n_live = torch.empty((1,), dtype=I32, device=dev)
        coords = torch.empty((cap, 4), dtype=I32, device=dev)
        part_rows = torch.empty((cap, 4), dtype=F32, device=dev)
        live_vox = torch.empty((cap,), dtype=I32, device=dev)
        feat_rows = torch.empty((cap, C), dtype=F32, device=dev)
        arg_rows = torch.empty((cap, C), dtype=I32, device=dev)
        src, stride, offset = (point_coords, 4, 1) if disable_part else (point_part_offset, 3, 0)
        _call("pda_parta2_pool_segments", point_coords, point_coords.data_ptr(), P, B, seg.data_ptr(),
              None if flag is None else flag.data_ptr())
        _call("pda_parta2_pool_collect", point_coords, rois.data_ptr(), point_coords.data_ptr(), seg.data_ptr(), table.data_ptr(), B, N, P,
              out, k_slots)
        _call("pda_parta2_pool_sparsify", point_coords, table.data_ptr(), src.data_ptr(), stride, offset, scores.data_ptr(), thresh,
              ws.data_ptr(), n_live.data_ptr(), coords.data_ptr(), part_rows.data_ptr(), live_vox.data_ptr(), total, P, out, k_slots)
        _call("pda_parta2_pool_features", point_coords, point_features.data_ptr(), table.data_ptr(), live_vox.data_ptr(),
              n_live.data_ptr(), feat_rows.data_ptr(), arg_rows.data_ptr(), total, P, C, out, k_slots)
        if check:
            n, bad = torch.cat((n_live, flag)).tolist()                             # the one host read
            if bad:
                raise ValueError("point_coords must be scene-major: a batch index in [0, %d) per row, ascending" % B)
        else:
            n = int(n_live.item())                                                  # the one host read
        ctx.save_for_backward(table, live_vox, arg_rows, scores)
        ctx.host = (thresh, k_slots, disable_part, n, P, C)
        coords = coords[:n]
        ctx.mark_non_differentiable(coords)
        return coords, part_rows[:n], feat_rows[:n]

    @staticmethod
    def backward(ctx, _g_coords, g_part, g_feat):
        table, live_vox, arg_rows, scores = ctx.saved_tensors
        thresh, k_slots, disable_part, n, P, C = ctx.host
        dev = table.device
        want_feat = ctx.needs_input_grad[0] and g_feat is not None
        want_part = ctx.needs_input_grad[1] and g_part is not None and not disable_part
        grad_feat = torch.zeros((P, C), dtype=F32, device=dev) if ctx.needs_input_grad[0] else None
        grad_off = torch.zeros((P, 3), dtype=F32, device=dev) if ctx.needs_input_grad[1] else None
        if n and P and (want_feat or want_part):
            g_part = g_part.contiguous() if want_part else None
            g_feat = g_feat.contiguous() if want_feat else None
            _call("pda_parta2_pool_bwd", table, table.data_ptr(), live_vox.data_ptr(), arg_rows.data_ptr(), scores.data_ptr(), thresh,
                  None if g_part is None else g_part.data_ptr(), None if g_feat is None else g_feat.data_ptr(),
                  None if grad_off is None else grad_off.data_ptr(), None if grad_feat is None else grad_feat.data_ptr(), n, P, C, k_slots)
        return grad_feat, grad_off, None, None, None, None


def parta2_pool(rois, point_coords, point_features, point_part_offset, point_cls_scores, thresh, pool_size, max_pts_each_voxel,
                disable_part=False, check=False):
    """The input stage of PartA2FCHead for the whole batch.  rois (B, N, >= 7), point_coords (P, 4) [bs_idx, x, y, z]
    scene-major, point_features (P, C), point_part_offset (P, 3), point_cls_scores (P) (detached here, as in the reference) ->
    (coords (n_live, 4) int32 [roi, x, y, z] in ascending order, part rows (n_live, 4), feature rows (n_live, C)).
    Differentiable in point_features and point_part_offset.  One host read: the count (with check=True also the flag that
    says whether point_coords is scene-major)."""
    out, k_slots = int(pool_size), int(max_pts_each_voxel)
    if rois.dim() != 3 or rois.shape[2] < 7 or point_coords.dim() != 2 or point_coords.shape[1] != 4:
        raise ValueError("rois must be (B, N, >= 7) and point_coords (P, 4), got %s and %s" % (tuple(rois.shape), tuple(point_coords.shape)))
    P = point_coords.shape[0]
    if point_features.dim() != 2 or point_features.shape[0] != P or tuple(point_part_offset.shape) != (P, 3) \
            or point_cls_scores.numel() != P or point_features.shape[1] < 1:
        raise ValueError("%d points with features %s, part offsets %s and scores %s" % (
            P, tuple(point_features.shape), tuple(point_part_offset.shape), tuple(point_cls_scores.shape)))
    if not 1 <= out <= MAX_POOL_SIZE or k_slots < 1:
        raise NotImplementedError("POOL_SIZE %d (1..%d) / MAX_POINTS_PER_VOXEL %d" % (out, MAX_POOL_SIZE, k_slots))
    rois7 = rois[..., 0:7].detach().contiguous()
    coords = point_coords.detach().contiguous()
    scores = point_cls_scores.detach().reshape(-1).contiguous()
    feats, offs = point_features.contiguous(), point_part_offset.contiguous()
    for name, t in (("rois", rois7), ("point_coords", coords), ("point_cls_scores", scores), ("point_features", feats),
                    ("point_part_offset", offs)):
        _chk(t, name, F32)
    return _PartA2Pool.apply(feats, offs, rois7, coords, scores, (float(thresh), out, k_slots, bool(disable_part), bool(check)))


def parta2_pool_composed(pool_layer, rois, point_coords, point_features, point_part_offset, point_cls_scores, thresh,
                         disable_part=False):
    """The same rows by the reference's order of work (partA2_head.py:104-197) on the existing operators: a boolean mask per
    scene, RoIAwarePool3d twice, nonzero() and indexing.  B + 1 host reads and two collection passes."""
    batch_idx, xyz = point_coords[:, 0], point_coords[:, 1:4]
    part_features = torch.cat((xyz if disable_part else point_part_offset, point_cls_scores.view(-1, 1).detach()), dim=1)
    part_features = torch.where((part_features[:, -1:] < thresh) & (torch.arange(4, device=xyz.device) < 3), torch.zeros_like(part_features),
                                part_features)
    pooled_part, pooled_rpn = [], []
    for bs_idx in range(rois.shape[0]):
        bs_mask = batch_idx == bs_idx
        cur_xyz, cur_roi = xyz[bs_mask].contiguous(), rois[bs_idx][:, 0:7].contiguous()
        pooled_part.append(pool_layer(cur_roi, cur_xyz, part_features[bs_mask], pool_method='avg'))
        pooled_rpn.append(pool_layer(cur_roi, cur_xyz, point_features[bs_mask], pool_method='max'))
    pooled_part, pooled_rpn = torch.cat(pooled_part, dim=0), torch.cat(pooled_rpn, dim=0)        # (B * N, P, P, P, 4 | C)
    idx = pooled_part.sum(dim=-1).nonzero()
    return idx.int().contiguous(), pooled_part[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]], \
        pooled_rpn[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]


class PartA2FCHead(RoIHeadTemplate):
    RCNN_KEYS = ('rcnn_subm1', 'rcnn_subm1_1', 'rcnn_subm2', 'rcnn_subm1_2')

    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.SA_modules = nn.ModuleList()
        pool_cfg = model_cfg['ROI_AWARE_POOL']
        block = self.post_act_block
        c0 = pool_cfg['NUM_FEATURES'] // 2
        self.conv_part = spconv.SparseSequential(block(4, 64, 3, padding=1, indice_key='rcnn_subm1'),
                                                 block(64, c0, 3, padding=1, indice_key='rcnn_subm1_1'))
        self.conv_rpn = spconv.SparseSequential(block(input_channels, 64, 3, padding=1, indice_key='rcnn_subm2'),
                                                block(64, c0, 3, padding=1, indice_key='rcnn_subm1_2'))
        pool_size = pool_cfg['POOL_SIZE']
        self.shared_fc_layer, pre_channel = self.make_shared_fc_layers(pool_cfg['NUM_FEATURES'] * pool_size ** 3, model_cfg['SHARED_FC'])
        self.cls_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=self.num_class, fc_list=model_cfg['CLS_FC'])
        self.reg_layers = self.make_fc_layers(input_channels=pre_channel, output_channels=self.box_coder.code_size * self.num_class,
                                              fc_list=model_cfg['REG_FC'])
        self.roiaware_pool3d_layer = RoIAwarePool3d(out_size=pool_size, max_pts_each_voxel=pool_cfg['MAX_POINTS_PER_VOXEL'])
        self.init_weights(weight_init='xavier')

    def post_act_block(self, in_channels, out_channels, kernel_size, indice_key, stride=1, padding=0, conv_type='subm'):
        if conv_type != 'subm':
            raise NotImplementedError("PartA2FCHead builds submanifold blocks only, not %r" % (conv_type,))
        return spconv.SparseSequential(spconv.SubMConv3d(in_channels, out_channels, kernel_size, bias=False, indice_key=indice_key),
                                       nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01), nn.ReLU())

    def roiaware_pool(self, batch_dict):
        """rois (B, num_rois, 7 + C), point_coords (P, 4) [bs_idx, x, y, z], point_features (P, C), point_cls_scores (P),
        point_part_offset (P, 3) -> (coords (n_live, 4) int32 [roi, x, y, z], part rows (n_live, 4), feature rows (n_live, C)):
        the rows the reference gathers from its dense pooled tensors at `sparse_idx`."""
        cfg = self.model_cfg
        args = (batch_dict['rois'], batch_dict['point_coords'], batch_dict['point_features'], batch_dict['point_part_offset'],
                batch_dict['point_cls_scores'], cfg['SEG_MASK_SCORE_THRESH'])
        disable_part = bool(cfg.get('DISABLE_PART', False))
        if fused_or_composed('PDA_PARTA2_POOL') == 'composed':
            return parta2_pool_composed(self.roiaware_pool3d_layer, *args, disable_part=disable_part)
        pool_cfg = cfg['ROI_AWARE_POOL']
        return parta2_pool(*args, pool_cfg['POOL_SIZE'], pool_cfg['MAX_POINTS_PER_VOXEL'], disable_part=disable_part,
                           check=bool(batch_dict.get('check_point_order', False)))

    @staticmethod
    def fake_sparse_idx(coords, part_rows, feat_rows, batch_size_rcnn):
        """At most two voxels are live: voxel (0, 0, 0) of every RoI stands in (BatchNorm needs two values a channel).  Its
        rows are what the dense pooled tensors hold there: a live voxel's own row, zeros elsewhere."""
        at_origin = (coords[:, 1:] == 0).all(dim=1, keepdim=True).to(part_rows.dtype)
        roi = coords[:, 0].long()
        fake_part = part_rows.new_zeros((batch_size_rcnn, part_rows.shape[1])).index_add(0, roi, part_rows * at_origin)
        fake_feat = feat_rows.new_zeros((batch_size_rcnn, feat_rows.shape[1])).index_add(0, roi, feat_rows * at_origin)
        fake = torch.zeros((batch_size_rcnn, 4), dtype=I32, device=coords.device)
        fake[:, 0] = torch.arange(batch_size_rcnn, dtype=I32, device=coords.device)
        return fake, fake_part, fake_feat

    def forward(self, batch_dict):
        targets_dict = self.proposals_and_targets(batch_dict)
        coords, part_rows, feat_rows = self.roiaware_pool(batch_dict)
        batch_size_rcnn = batch_dict['rois'].shape[0] * batch_dict['rois'].shape[1]
        pool_size = self.model_cfg['ROI_AWARE_POOL']['POOL_SIZE']
        sparse_shape = [pool_size] * 3
        if coords.shape[0] < 3:                                     # decided on the host, from the count already read
            coords, part_rows, feat_rows = self.fake_sparse_idx(coords, part_rows, feat_rows, batch_size_rcnn)
            if self.training:                                       # these are invalid samples
                targets_dict['rcnn_cls_labels'].fill_(-1)
                targets_dict['reg_valid_mask'].fill_(-1)

        # the four submanifold layers see the same sites with the same kernel: one rulebook under their four keys
        book = spconv.build_subm_rulebook(coords, sparse_shape, batch_size_rcnn, 3)
        books = {key: book for key in self.RCNN_KEYS}
        part_features = spconv.SparseConvTensor(part_rows, coords, sparse_shape, batch_size_rcnn, books)
        rpn_features = spconv.SparseConvTensor(feat_rows, coords, sparse_shape, batch_size_rcnn, books)
        x_part = self.conv_part(part_features)
        x_rpn = self.conv_rpn(rpn_features)

        merged_feature = torch.cat((x_rpn.features, x_part.features), dim=1)
        shared_feature = spconv.SparseConvTensor(merged_feature, coords, sparse_shape, batch_size_rcnn)
        shared_feature = shared_feature.dense().view(batch_size_rcnn, -1, 1)
        shared_feature = self.shared_fc_layer(shared_feature)
        rcnn_cls = self.cls_layers(shared_feature).transpose(1, 2).contiguous().squeeze(dim=1)            # (B, 1 or 2)
        rcnn_reg = self.reg_layers(shared_feature).transpose(1, 2).contiguous().squeeze(dim=1)            # (B, C)
        return self.keep_predictions(batch_dict, targets_dict, rcnn_cls, rcnn_reg)
