#!/usr/bin/env python
"""Generates tests/golden/roi_targets.npz: the REFERENCE's RoI-head front end run on synthetic batches on CPU tensors --
RoIHeadTemplate.proposal_layer, assign_targets (ProposalTargetLayer and the canonical transformation),
generate_predicted_boxes and get_loss (pcdet/models/roi_heads/roi_head_template.py,
roi_heads/target_assigner/proposal_target_layer.py), ResidualCoder (pcdet/utils/box_coder_utils.py) and the state-dict keys
of make_fc_layers.

The two modules are loaded through reference_loader.py; pcdet/utils/{common_utils, box_utils, box_coder_utils,
loss_utils}.py, model_nms_utils.py and iou3d_nms_utils.py are the reference's own files, iou3d_nms_cuda is the repository's C
oracle (oracle/: boxes_overlap_bev_gpu, nms_gpu); in proposal_target_layer.py torch.cat reads the `[]` of the fg-only branch
as an empty index tensor (this torch refuses a list there).  np.random.permutation, np.random.rand and torch.randint are wrapped to record each scene's draws, which the
fixture stores padded per scene so that the explicit mode of pda_roi_sample_targets can repeat them.

Stored per target batch b<i>_: case, cfg (json of TARGET_CONFIG), rois, roi_scores, roi_labels, gt_boxes, the draws
(perm, fg_rand, hard_draw, easy_draw and their per-scene counts), max_overlaps / gt_assignment per scene and the targets
dict after assign_targets (t_<key>).  Loss cases l<i>_: the batch they use, LOSS_CONFIG, rcnn_cls / rcnn_reg, the loss, the
tb_dict and both gradients.  Proposal cases p<i>_: layout, nms_cfg, the predictions, gt_boxes, rois / roi_scores /
roi_labels.  Coverage is asserted with roi_targets_cover.py.

Run with the reference checkout:  python tests/golden/make_roi_targets_golden.py /path/to/reference
"""
import contextlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from reference_loader import MODEL_UTILS, ROI_HEAD, cpu_torch, extension_stubs, load, reference_root  # noqa: E402
from pdanet_amd.config import to_attr  # noqa: E402
import roi_targets_cover as cover  # noqa: E402

OUT = os.path.join(HERE, "roi_targets.npz")
IOU = PTL = RHT = CODER = None   # the reference's iou3d_nms_utils, proposal_target_layer, roi_head_template and box_coder_utils


class _CpuTorch(types.ModuleType):
    """torch, with cuda.FloatTensor(size) a CPU float32 tensor (boxes_iou3d_gpu allocates its BEV plane so)."""

    def __getattr__(self, name):
        return getattr(torch, name)


def load_reference(root):
    """Loads the reference's utils, NMS, proposal_target_layer and roi_head_template as pcdet_ref.* and binds IOU, PTL, RHT and
    CODER to them."""
    global IOU, PTL, RHT, CODER
    cpu_torch()
    utils = dict(zip(MODEL_UTILS, load(root, "pcdet_ref", MODEL_UTILS, stubs=extension_stubs())))
    IOU, CODER = utils["ops.iou3d_nms.iou3d_nms_utils"], utils["utils.box_coder_utils"]
    ct = _CpuTorch("torch")
    ct.cuda = types.SimpleNamespace(FloatTensor=lambda size: torch.empty(size, dtype=torch.float32))
    IOU.torch = ct
    PTL = load(root, "pcdet_ref", ROI_HEAD[:2])[1]
    # subsample_rois' fg-only branch ends in torch.cat((fg_inds, [])), which this torch refuses; an empty list element is
    # read as the empty index tensor it stands for, so that the branch yields the fg picks it computed
    pt = _CpuTorch("torch")
    pt.cat = lambda ts, dim=0: torch.cat([t if isinstance(t, torch.Tensor) else torch.zeros(0, dtype=torch.long) for t in ts], dim=dim)
    PTL.torch = pt
    RHT, = load(root, "pcdet_ref", ROI_HEAD[2:])


@contextlib.contextmanager
def recording(log):
    """log: a list that receives (name, array) for every draw the reference makes."""
    perm, rand, randint = np.random.permutation, np.random.rand, torch.randint

    def _perm(n):
        r = perm(n)
        log.append(('perm', np.asarray(r).copy()))
        return r

    def _rand(*shape):
        r = rand(*shape)
        log.append(('fg_rand', np.asarray(r).copy()))
        return r

    def _randint(*a, **k):
        r = randint(*a, **k)
        log.append(('randint', r.numpy().copy(), int(k['high'])))   # the reference passes low / high / size by name
        return r

    np.random.permutation, np.random.rand, torch.randint = _perm, _rand, _randint
    try:
        yield
    finally:
        np.random.permutation, np.random.rand, torch.randint = perm, rand, randint


LOSS_WEIGHTS = {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0, 'code_weights': [1.0] * 7}


def model_cfg(target_cfg, cls_loss='BinaryCrossEntropy', corner=True):
    return to_attr({'TARGET_CONFIG': dict(target_cfg, BOX_CODER='ResidualCoder'), 'DP_RATIO': 0.3,
                    'LOSS_CONFIG': {'CLS_LOSS': cls_loss, 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': corner,
                                    'LOSS_WEIGHTS': LOSS_WEIGHTS}})


BASE = {'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5, 'SAMPLE_ROI_BY_EACH_CLASS': True, 'CLS_SCORE_TYPE': 'cls', 'CLS_FG_THRESH': 0.6,
        'CLS_BG_THRESH': 0.45, 'CLS_BG_THRESH_LO': 0.1, 'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55}
CONFIGS = {
    'pointrcnn': dict(BASE),
    'pvrcnn': dict(BASE, CLS_SCORE_TYPE='roi_iou', CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25),
    'agnostic': dict(BASE, SAMPLE_ROI_BY_EACH_CLASS=False, ROI_PER_IMAGE=32),
    'overlap': dict(BASE, CLS_FG_THRESH=0.5, CLS_BG_THRESH=0.3, ROI_PER_IMAGE=32),
    'exact_cls': dict(BASE, CLS_FG_THRESH=0.5, REG_FG_THRESH=0.5, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.125, ROI_PER_IMAGE=32),
    'exact_iou': dict(BASE, CLS_SCORE_TYPE='roi_iou', CLS_FG_THRESH=0.5, REG_FG_THRESH=0.5, CLS_BG_THRESH=0.25,
                      CLS_BG_THRESH_LO=0.125, ROI_PER_IMAGE=32),
}


def reference_max_iou(rois, labels, gt, by_class):
    """Per scene, the reference's own functions on the GT trimmed as it trims it."""
    B, M = rois.shape[:2]
    mo, ga = np.zeros((B, M), np.float32), np.zeros((B, M), np.int32)
    for s in range(B):
        g = torch.from_numpy(gt[s, :cover.kept_rows(gt[s])])
        r, l = torch.from_numpy(rois[s]), torch.from_numpy(labels[s])
        if by_class:
            o, a = PTL.ProposalTargetLayer.get_max_iou_with_same_class(rois=r, roi_labels=l, gt_boxes=g[:, 0:7], gt_labels=g[:, -1].long())
        else:
            o, a = torch.max(IOU.boxes_iou3d_gpu(r, g[:, 0:7]), dim=1)
        mo[s], ga[s] = o.numpy(), a.numpy()
    return mo, ga


def run_targets(name, cfg, rois, scores, labels, gt):
    """assign_targets of the reference over one batch -> the fixture entries of the batch and the targets dict."""
    B, M = rois.shape[:2]
    R = cfg['ROI_PER_IMAGE']
    head = RHT.RoIHeadTemplate(num_class=3, model_cfg=model_cfg(cfg))
    mo, ga = reference_max_iou(rois, labels, gt, cfg['SAMPLE_ROI_BY_EACH_CLASS'])
    draws = {'perm': np.zeros((B, M), np.int32), 'fg_rand': np.zeros((B, R), np.float64),
             'hard_draw': np.zeros((B, R), np.int64), 'easy_draw': np.zeros((B, R), np.int64)}
    counts = np.zeros((B, 4), np.int32)                  # valid entries of perm, fg_rand, hard_draw, easy_draw
    logs = []
    real_subsample = PTL.ProposalTargetLayer.subsample_rois

    def subsample(self, max_overlaps):
        logs.append([])
        with recording(logs[-1]):
            return real_subsample(self, max_overlaps)

    PTL.ProposalTargetLayer.subsample_rois = subsample
    try:
        bd = {'batch_size': B, 'rois': torch.from_numpy(rois.copy()), 'roi_scores': torch.from_numpy(scores.copy()),
              'roi_labels': torch.from_numpy(labels.copy()), 'gt_boxes': torch.from_numpy(gt.copy())}
        targets = head.assign_targets(bd)
    finally:
        PTL.ProposalTargetLayer.subsample_rois = real_subsample
    assert len(logs) == B
    for s, log in enumerate(logs):
        fg, hard, easy = cover.category_counts(mo[s], cfg)
        assert fg.sum() + hard.sum() + easy.sum() > 0
        ints = [e for e in log if e[0] == 'randint']
        order = (['hard_draw', 'easy_draw'] if hard.any() and easy.any() else ['hard_draw'] if hard.any() else ['easy_draw'])
        assert len(ints) == (len(order) if hard.any() or easy.any() else 0), (name, s, len(ints))
        for key, e in zip(order, ints):
            assert e[2] == (hard.sum() if key == 'hard_draw' else easy.sum())
            draws[key][s, :len(e[1])] = e[1]
            counts[s, 2 if key == 'hard_draw' else 3] = len(e[1])
        for e in log:
            if e[0] == 'perm':
                assert len(e[1]) == fg.sum()
                draws['perm'][s, :len(e[1])] = e[1]
                counts[s, 0] = len(e[1])
            elif e[0] == 'fg_rand':
                draws['fg_rand'][s, :len(e[1])] = e[1]
                counts[s, 1] = len(e[1])
    out = {'case': np.array(name), 'cfg': np.array(json.dumps(cfg)), 'rois': rois, 'roi_scores': scores, 'roi_labels': labels,
           'gt_boxes': gt, 'max_overlaps': mo, 'gt_assignment': ga, 'draw_counts': counts}
    out.update(draws)
    for k, v in targets.items():
        out['t_' + k] = v.numpy().copy()
    return out, head, targets


# ---- scenes ------------------------------------------------------------------------------------------------------------
DIMS = {1: (3.9, 1.6, 1.56), 2: (0.8, 0.6, 1.73), 3: (1.76, 0.6, 1.73)}


def gt_rows(rng, n, label_set):
    """n GT rows on a jittered 8 m grid (so that a RoI overlaps the box it was made from and no other)."""
    cells = rng.permutation(100)[:n]
    g = np.zeros((n, 8), np.float32)
    cls = rng.choice(sorted(label_set), n)
    g[:, 0] = (cells % 10 - 4.5) * 8 + rng.uniform(-1, 1, n)
    g[:, 1] = (cells // 10 - 4.5) * 8 + rng.uniform(-1, 1, n)
    g[:, 2] = rng.uniform(-1.8, -0.5, n)
    g[:, 3:6] = np.array([DIMS[c] for c in cls]) * rng.uniform(0.85, 1.15, (n, 3))
    g[:, 6] = rng.uniform(-np.pi, np.pi, n)
    g[:, 7] = cls
    near = rng.random(n) < 0.2                           # headings next to +-pi
    g[near, 6] = np.where(rng.random(near.sum()) < 0.5, np.pi, -np.pi) - np.sign(rng.standard_normal(near.sum())) * 1e-4
    return g


def roi_of(rng, g, kind, free):
    """A RoI made from GT row g by sliding it a fraction f of its length along its own axis: with the same size and heading
    the IoU is (1 - f) / (1 + f).  kind 'fg' f <= 0.25 (IoU >= 0.6), 'hard' 0.32..0.75 (0.14..0.52), 'easy' >= 0.9 (< 0.06).
    free: also perturb heading and size a little (the category may then move across a threshold; the scenes that need an
    exact branch do not use it).  The heading is turned by whole multiples of pi, which leaves the geometry alone and
    moves GT-minus-RoI across the fold branches and the RoI heading below 0 and above 2 pi."""
    f = {'fg': rng.uniform(0, 0.25), 'hard': rng.uniform(0.32, 0.75), 'easy': rng.uniform(0.9, 2.5),
         'mid': rng.uniform(0.295, 0.33)}[kind]      # 'mid': IoU in (0.5, 0.545), fg and hard_bg at once under 'overlap'
    r = g[:7].astype(np.float64).copy()
    r[0] += f * g[3] * np.cos(g[6])
    r[1] += f * g[3] * np.sin(g[6])
    if free:
        r[6] += rng.uniform(-0.06, 0.06)
        r[3:6] *= rng.uniform(0.97, 1.03, 3)
    r[6] += rng.choice([0, 0, 0, 1, -1, 2, -2, 3]) * np.pi
    return r.astype(np.float32)


def scene(rng, M, T, n_gt, label_set, n_fg, n_hard, n_easy, n_mid=0, n_far=0, n_wrong=0, n_zero=0, free=True, zero_mid=False,
          dup=False, trailing=False, other_label=None):
    """One scene: (rois (M, 7), scores (M), labels (M) int64, gt (T, 8)).  n_wrong RoIs sit on a GT box but carry
    other_label, a class the scene has no GT of; n_far lie away from every GT; n_zero rows are zero padding."""
    assert n_fg + n_hard + n_easy + n_mid + n_far + n_wrong + n_zero == M
    g = gt_rows(rng, n_gt, label_set)
    rows, labels = [], []
    for kind, n in (('fg', n_fg), ('hard', n_hard), ('easy', n_easy), ('mid', n_mid)):
        for _ in range(n):
            j = rng.integers(0, n_gt)
            rows.append(roi_of(rng, g[j], kind, free))
            labels.append(int(g[j, 7]))
    for _ in range(n_wrong):
        j = rng.integers(0, n_gt)
        rows.append(roi_of(rng, g[j], 'fg', free))
        labels.append(other_label)
    for _ in range(n_far):
        far = gt_rows(rng, 1, label_set)[0]
        far[0:2] += np.float32(200.0)
        rows.append(far[:7])
        labels.append(int(far[7]))
    order = rng.permutation(len(rows))
    rois = np.zeros((M, 7), np.float32)
    lab = np.ones(M, np.int64)                           # zero padding carries label 1, as proposal_layer leaves it
    if rows:
        rois[:len(rows)] = np.array(rows, np.float32)[order]
        lab[:len(rows)] = np.array(labels, np.int64)[order]
    scores = np.zeros(M, np.float32)
    scores[:len(rows)] = np.sort(rng.standard_normal(len(rows)).astype(np.float32))[::-1]
    gt = np.zeros((T, 8), np.float32)
    gt[:n_gt] = g
    if dup:                                              # the same box twice: the arg-max tie
        assert n_gt + 2 <= T
        gt[n_gt], gt[n_gt + 1] = g[0], g[1]
    if zero_mid:
        gt[1] = 0
    if trailing:
        gt[T - 1] = g[0] if not dup else g[2]
    return rois, scores, lab, gt


def all_zero_gt(sc):
    """The scene with every GT row zero: the reference keeps row 0, one zero box with label 0."""
    return sc[:3] + (np.zeros_like(sc[3]),)


def stack(scenes):
    return tuple(np.stack([s[i] for s in scenes]) for i in range(4))


def exact_scene(M, T, shift):
    """Axis-aligned nested boxes: a RoI with the GT's height strictly inside a 4 x 5 x 2 GT has IoU = its BEV area / 20:
    2.5 x 4 -> 0.5, 2 x 2.5 -> 0.25, 1 x 2.5 -> 0.125 exactly; 4 x 4.5 -> 0.9, 0.5 x 2 -> 0.05, the GT itself -> 1.  Every
    RoI appears centred and moved by a quarter (still nested for the three exact sizes)."""
    gt = np.zeros((T, 8), np.float32)
    centres = [(10 + shift, 5), (-12, 8 - shift), (30, -20 + shift), (-30 - shift, -25)]
    for j, (x, y) in enumerate(centres):
        gt[j] = [x, y, -1, 4, 5, 2, 0, 1 + j % 3]
    sizes = [(2.5, 4), (2, 2.5), (1, 2.5), (4, 4.5), (0.5, 2), (4, 5)]
    rows, labels = [], []
    for j, (x, y) in enumerate(centres):
        for dx, dy in sizes:
            for off in ((0, 0), (0.25, -0.25)):
                rows.append([x + off[0], y + off[1], -1, dx, dy, 2, 0])
                labels.append(1 + j % 3)
    assert len(rows) <= M - 8
    rois = np.zeros((M, 7), np.float32)
    lab = np.ones(M, np.int64)
    rois[:len(rows)] = np.array(rows, np.float32)
    lab[:len(rows)] = labels
    scores = np.linspace(3, -3, M).astype(np.float32)
    return rois, scores, lab, gt


def proposal_inputs(rng, B, N, T):
    gt = np.zeros((B, T, 8), np.float32)
    box = np.zeros((B, N, 7), np.float32)
    cls = np.zeros((B, N, 3), np.float32)
    for s in range(B):
        g = gt_rows(rng, 5, {1, 2, 3})
        gt[s, :5] = g
        for i in range(N):
            j = rng.integers(0, 5)
            box[s, i] = roi_of(rng, g[j], rng.choice(['fg', 'fg', 'hard', 'easy']), True)
        cls[s] = rng.standard_normal((N, 3)).astype(np.float32) * 2
        assert len(np.unique(cls[s].max(axis=1))) == N   # distinct scores: topk and sort order equal ones differently
    return box, cls, gt


def main():
    load_reference(reference_root())
    rng = np.random.default_rng(20261018)
    np.random.seed(7)
    torch.manual_seed(7)
    batches = []
    # pointrcnn: B 4, M 512, T 64, R 128 (quota 64)
    batches.append(('pointrcnn', stack([
        scene(rng, 512, 64, 40, {1, 2, 3}, 150, 150, 150, n_far=30, n_zero=32, zero_mid=True, dup=True),     # fg above quota
        scene(rng, 512, 64, 30, {1, 3}, 20, 12, 300, n_far=100, n_wrong=40, n_zero=40, other_label=2),       # fg, hard below
        scene(rng, 512, 64, 63, {1, 2, 3}, 512, 0, 0, free=False, trailing=True),                            # fg only
        all_zero_gt(scene(rng, 512, 64, 10, {1, 2}, 100, 100, 200, n_zero=112)),
    ])))
    batches.append(('pointrcnn', stack([                 # a second batch of the same shapes
        scene(rng, 512, 64, 20, {2, 3}, 40, 200, 200, n_far=40, n_zero=32),
        scene(rng, 512, 64, 50, {1, 2, 3}, 300, 100, 80, n_zero=32, dup=True, trailing=True),
        scene(rng, 512, 64, 12, {1, 2, 3}, 0, 256, 224, n_zero=32),                                          # bg only, both lists
        scene(rng, 512, 64, 33, {1, 3}, 64, 64, 300, n_wrong=44, n_zero=40, other_label=2),
    ])))
    # pvrcnn: B 4, M 128, T 16, R 128, roi_iou
    batches.append(('pvrcnn', stack([
        scene(rng, 128, 16, 8, {1, 2, 3}, 40, 40, 40, n_zero=8, zero_mid=True),
        scene(rng, 128, 16, 10, {1, 2, 3}, 0, 128, 0, free=False),                                           # hard only
        scene(rng, 128, 16, 6, {1, 3}, 0, 60, 40, n_wrong=20, n_zero=8, other_label=2),                      # bg only
        scene(rng, 128, 16, 12, {1, 2, 3}, 10, 8, 90, n_far=12, n_zero=8, dup=True, trailing=True),          # hard below quota
    ])))
    # agnostic: B 2, M 64, T 8, R 32
    batches.append(('agnostic', stack([
        scene(rng, 64, 8, 5, {1, 2, 3}, 20, 20, 16, n_zero=8, dup=True),
        scene(rng, 64, 8, 4, {1, 3}, 6, 10, 30, n_wrong=10, n_zero=8, other_label=2, trailing=True),
    ])))
    # overlap: B 3, M 128, T 16, R 32; fg and hard_bg share the RoIs with 0.5 <= IoU < 0.55
    batches.append(('overlap', stack([
        scene(rng, 128, 16, 8, {1, 2, 3}, 40, 40, 20, n_mid=20, n_zero=8, free=False),
        scene(rng, 128, 16, 8, {1, 2, 3}, 30, 70, 20, n_zero=8, zero_mid=True),
        scene(rng, 128, 16, 8, {1, 3}, 60, 30, 20, n_wrong=10, n_zero=8, other_label=2),
    ])))
    for name in ('exact_cls', 'exact_iou'):
        batches.append((name, stack([exact_scene(64, 8, 0), exact_scene(64, 8, 2)])))

    out = {'n_batches': np.int64(len(batches))}
    kept = {}
    for i, (name, (rois, scores, labels, gt)) in enumerate(batches):
        entries, head, targets = run_targets(name, CONFIGS[name], rois, scores, labels, gt)
        for k, v in entries.items():
            out['b%d_%s' % (i, k)] = v
        kept[i] = (head, entries)
        print(name, rois.shape, gt.shape, [tuple(int(m.sum()) for m in cover.category_counts(entries['max_overlaps'][s], CONFIGS[name]))
                                           for s in range(rois.shape[0])])

    # losses and box decoding on the targets of four batches
    # (BinaryCrossEntropy goes with 'roi_iou' targets only: this torch's binary_cross_entropy refuses the -1 of 'cls')
    loss_cases = [(2, 'BinaryCrossEntropy', True), (0, 'CrossEntropy', True), (6, 'BinaryCrossEntropy', False), (3, 'CrossEntropy', False)]
    out['n_loss'] = np.int64(len(loss_cases))
    for i, (b, cls_loss, corner) in enumerate(loss_cases):
        entries = kept[b][1]
        cfg = json.loads(str(entries['cfg']))
        head = RHT.RoIHeadTemplate(num_class=3, model_cfg=model_cfg(cfg, cls_loss, corner))
        n = entries['t_rois'].shape[0] * entries['t_rois'].shape[1]
        rcnn_cls = torch.from_numpy(rng.standard_normal((n, 2 if cls_loss == 'CrossEntropy' else 1)).astype(np.float32)).requires_grad_(True)
        rcnn_reg = torch.from_numpy((rng.standard_normal((n, 7)) * 0.3).astype(np.float32)).requires_grad_(True)
        fr = {k[2:]: torch.from_numpy(v.copy()) for k, v in entries.items() if k.startswith('t_')}   # encode_torch writes into them
        fr.update(rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg)
        head.forward_ret_dict = fr
        loss, tb = head.get_loss()
        loss.backward()
        p = 'l%d_' % i
        out[p + 'batch'] = np.int64(b)
        out[p + 'loss_cfg'] = np.array(json.dumps({'CLS_LOSS': cls_loss, 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': corner,
                                                   'LOSS_WEIGHTS': LOSS_WEIGHTS}))
        out[p + 'rcnn_cls'], out[p + 'rcnn_reg'] = rcnn_cls.detach().numpy(), rcnn_reg.detach().numpy()
        out[p + 'loss'] = loss.detach().numpy()
        out[p + 'tb_keys'] = np.array(list(tb.keys()), dtype='<U40')
        out[p + 'tb_vals'] = np.array([tb[k] for k in tb], np.float64)
        out[p + 'grad_cls'], out[p + 'grad_reg'] = rcnn_cls.grad.numpy(), rcnn_reg.grad.numpy()
        with torch.no_grad():
            bc, bb = head.generate_predicted_boxes(entries['t_rois'].shape[0], torch.from_numpy(entries['t_rois'].copy()),
                                                   rcnn_cls.detach(), rcnn_reg.detach())
        out[p + 'pred_cls'], out[p + 'pred_boxes'] = bc.numpy(), bb.numpy()
        print('loss', i, float(loss), tb)

    # proposal_layer: N 256, NMS_PRE_MAXSIZE 100, NMS_POST_MAXSIZE 32 and 512; one case per input layout
    head = kept[0][0]
    cases = [('3d', 32), ('batch_index', 512), ('3d', 32)]
    out['n_proposal'] = np.int64(len(cases))
    for i, (layout, post) in enumerate(cases):
        box, cls, gt = proposal_inputs(rng, 2, 256, 8)
        nms_cfg = {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 100, 'NMS_POST_MAXSIZE': post, 'NMS_THRESH': 0.8}
        bd = {'batch_size': 2, 'cls_preds_normalized': False}
        if layout == '3d':
            bd.update(batch_box_preds=torch.from_numpy(box.copy()), batch_cls_preds=torch.from_numpy(cls.copy()))
        else:
            bd.update(batch_box_preds=torch.from_numpy(box.reshape(-1, 7).copy()), batch_cls_preds=torch.from_numpy(cls.reshape(-1, 3).copy()),
                      batch_index=torch.arange(2).repeat_interleave(256).float())
        bd = head.proposal_layer(bd, to_attr(nms_cfg))
        assert 'batch_index' not in bd and bd['has_class_labels'] is True
        p = 'p%d_' % i
        out[p + 'layout'], out[p + 'nms_cfg'] = np.array(layout), np.array(json.dumps(nms_cfg))
        out[p + 'box_preds'], out[p + 'cls_preds'], out[p + 'gt_boxes'] = box, cls, gt
        out[p + 'rois'], out[p + 'roi_scores'], out[p + 'roi_labels'] = bd['rois'].numpy(), bd['roi_scores'].numpy(), bd['roi_labels'].numpy()
        print('proposal', layout, post, bd['rois'].numpy().any(axis=2).sum(axis=1))

    # ResidualCoder, both angle codes
    n = 64
    g = gt_rows(rng, n, {1, 2, 3})[:, :7]
    a = np.stack([roi_of(rng, r, 'fg', True) for r in g])
    a[0, 3:6] = 0                                        # a size below the clamp
    for tag, sincos in (('res', False), ('sincos', True)):
        coder = CODER.ResidualCoder(encode_angle_by_sincos=sincos)
        codes = coder.encode_torch(torch.from_numpy(g.copy()), torch.from_numpy(a.copy()))
        anchors = torch.from_numpy(a.copy())
        anchors[:, 3:6] = anchors[:, 3:6].clamp(min=1e-5)
        out['coder_%s_codes' % tag] = codes.numpy()
        out['coder_%s_decoded' % tag] = coder.decode_torch(codes, anchors).numpy()
    out['coder_boxes'], out['coder_anchors'] = g, a
    fc = head.make_fc_layers(input_channels=128, output_channels=7, fc_list=[256, 256])
    out['fc_keys'] = np.array(list(fc.state_dict().keys()), dtype='<U60')
    out['fc_modules'] = np.array([type(m).__name__ for m in fc], dtype='<U20')

    seen, shapes = cover.coverage(out)
    assert not cover.REQUIRED - seen, sorted(cover.REQUIRED - seen)
    for k, want in cover.SHAPES.items():
        assert shapes[k] <= want and len(shapes[k]) >= 2, (k, shapes[k])
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 1 << 20


if __name__ == "__main__":
    main()
