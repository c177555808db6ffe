// roi_targets.hip -- the training-side front end of a two-stage RoI head on the device: ProposalTargetLayer
// (roi_heads/target_assigner/proposal_target_layer.py) and the canonical transformation of RoIHeadTemplate.assign_targets
// (roi_head_template.py:104-134) for every scene of a batch in two launches and without a host read.
//
// Reference, per scene: trim the GT, then per class a boxes_iou3d_gpu (a dozen launches) behind two .item() reads, three
// nonzero() (a host synchronisation each), draws from numpy and torch's CPU generator uploaded per scene, and an
// advanced-indexing gather per output.
//
// Here: pda_roi_max_iou, one wave per (scene, RoI) whose lanes stride over the kept GT rows and reduce (IoU, lowest row);
// pda_roi_sample_targets, one workgroup per scene: three waves compact the fg / hard-bg / easy-bg lists in ascending RoI
// order with ballots (no atomics, so the lists do not depend on execution order), the branch rules of subsample_rois /
// sample_bg_inds are evaluated on wave-uniform counts, and each thread then gathers, labels and transforms one pick.
#include "pda_common.h"
#include "bev_overlap.h"
#include "box_iou3d.h"
#include "stage_rng.h"

#include <limits.h>

namespace pda {
namespace {

constexpr int ROI_MAX_M = 4096;          // RoIs a scene: three int32 lists of that length in LDS (48 KiB)
constexpr int ROI_IOU_WAVES = 4;         // RoIs per workgroup of the IoU kernel
constexpr int ROI_SAMPLE_THREADS = 256;
// stream_key purposes of the seeded mode (0..2 belong to the data stages)
constexpr int PURPOSE_FG = 3, PURPOSE_HARD = 4, PURPOSE_EASY = 5;

// get_max_iou_with_same_class / torch.max(boxes_iou3d_gpu(rois, gt), dim=1) of one RoI: the max over the kept GT rows
// (of the RoI's class when by_class) with the lowest row among equal maxima, as torch's CPU max keeps the first; 0 / 0
// without a row of that class, which is what the reference's per-class loop leaves in its zero-filled outputs.
__global__ __launch_bounds__(64 * ROI_IOU_WAVES) void roi_max_iou_kernel(
        const float* __restrict__ rois, const int64_t* __restrict__ roi_labels, const float* __restrict__ gt, int cols,
        int by_class, float* __restrict__ max_overlaps, int32_t* __restrict__ gt_assignment, int m, int t) {
    const int s = blockIdx.y, wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int i = (int)blockIdx.x * ROI_IOU_WAVES + wave;
    if (i >= m) return;  // the whole wave
    const float* sgt = gt + (size_t)s * t * cols;
    const int kept = t > 0 ? trimmed_last_row(sgt, t, cols, lane) + 1 : 0;  // t == 0: the reference's one zero box, IoU 0
    const float* ra = rois + ((size_t)s * m + i) * 7;
    const IouSide a = make_iou_side(ra);
    const BevBox abev = make_box(ra);
    const int64_t label = by_class ? roi_labels[(size_t)s * m + i] : 0;
    float best = -INFINITY;
    int arg = INT_MAX;
    for (int j = lane; j < kept; j += 64) {
        const float* gb = sgt + (size_t)j * cols;
        if (by_class && (int64_t)gb[cols - 1] != label) continue;  // cur_gt[:, -1].long()
        const IouSide b = make_iou_side(gb);
        const float iou = iou3d_apart(a, b) ? 0.f : iou3d_from_overlap(a, b, box_overlap(abev, make_box(gb)));
        if (arg == INT_MAX || iou > best) {  // ascending j within a lane: the first of equal values stays
            best = iou;
            arg = j;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float v = __shfl_xor(best, o);
        const int vi = __shfl_xor(arg, o);
        if (vi != INT_MAX && (arg == INT_MAX || v > best || (v == best && vi < arg))) {
            best = v;
            arg = vi;
        }
    }
    if (lane == 0) {
        max_overlaps[(size_t)s * m + i] = arg == INT_MAX ? 0.f : best;
        gt_assignment[(size_t)s * m + i] = arg == INT_MAX ? 0 : arg;
    }
}

struct RoiSampler {
    int roi_per_image, fg_per_image, score_type;      // fg_per_image = int(np.round(FG_RATIO * ROI_PER_IMAGE)), from the host
    double hard_bg_ratio;
    float reg_fg, cls_fg, cls_bg, cls_bg_lo, fg_thresh;  // float32 roundings: torch compares a float32 tensor in float32
    float fg_minus_bg;                                   // float32(CLS_FG_THRESH - CLS_BG_THRESH), the difference in double
};

struct RoiDraws {
    const int32_t* perm;       // (b, m)  np.random.permutation(fg_num)
    const double* fg_rand;     // (b, r)  np.random.rand(r)
    const int64_t* hard_draw;  // (b, r)  torch.randint(0, len(hard))
    const int64_t* easy_draw;  // (b, r)
    unsigned long long seed;
    int explicit_draws;
};

struct RoiTargetsOut {
    float* rois;
    float* gt_of_rois_src;
    float* gt_of_rois;
    float* gt_iou;
    float* roi_scores;
    int64_t* roi_labels;
    int64_t* reg_valid_mask;
    void* rcnn_cls_labels;  // int64 ('cls') or float32 ('roi_iou')
    int32_t* sampled_inds;  // optional
    int32_t* status;
};

// torch's float32 remainder: fmodf, then the divisor is added when the signs differ
__device__ __forceinline__ float torch_mod(float a, float b) {
    float r = fmodf(a, b);
    if (r != 0.f && ((b < 0.f) != (r < 0.f))) r += b;
    return r;
}

// NaN by its bits: the library is built with -fno-honor-nans, under which a float comparison of a NaN is undefined, and a
// scene of NaN IoUs has to land in none of the three lists as it does in the reference
// one compacted list: lanes of one wave walk the RoIs in ascending order; returns the list's length
template <typename Pred>
__device__ int compact_list(int* __restrict__ list, int m, int lane, Pred pred) {
    int n = 0;
    for (int base = 0; base < m; base += 64) {
        const int i = base + lane;
        const bool in = i < m && pred(i);
        const uint64_t mask = __ballot(in);
        if (in) list[n + rank_below(mask)] = i;
        n += __popcll(mask);
    }
    return n;
}

__global__ __launch_bounds__(ROI_SAMPLE_THREADS) void roi_sample_targets_kernel(
        const float* __restrict__ rois, const float* __restrict__ roi_scores, const int64_t* __restrict__ roi_labels,
        const float* __restrict__ gt, int cols, const float* __restrict__ max_overlaps,
        const int32_t* __restrict__ gt_assignment, RoiSampler cfg, RoiDraws dr, RoiTargetsOut out, int m, int t) {
    __shared__ int lists[3][ROI_MAX_M];  // fg, hard bg, easy bg
    __shared__ int counts[3];
    __shared__ int bad;
    const int s = blockIdx.x, wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int R = cfg.roi_per_image;
    const float* ov = max_overlaps + (size_t)s * m;
    if (threadIdx.x == 0) bad = 0;
    // the masks are literal (:117-125): with CLS_FG_THRESH < REG_FG_THRESH a RoI is in both fg and hard_bg
    if (wave == 0) {
        const int n = compact_list(lists[0], m, lane, [&](int i) { return !is_nan_bits(ov[i]) && ov[i] >= cfg.fg_thresh; });
        if (lane == 0) counts[0] = n;
    } else if (wave == 1) {
        const int n = compact_list(lists[1], m, lane, [&](int i) { return !is_nan_bits(ov[i]) && ov[i] < cfg.reg_fg && ov[i] >= cfg.cls_bg_lo; });
        if (lane == 0) counts[1] = n;
    } else if (wave == 2) {
        const int n = compact_list(lists[2], m, lane, [&](int i) { return !is_nan_bits(ov[i]) && ov[i] < cfg.cls_bg_lo; });
        if (lane == 0) counts[2] = n;
    }
    __syncthreads();
    const int fg_num = counts[0], hard_num = counts[1], easy_num = counts[2];
    const int bg_num = hard_num + easy_num;

    // subsample_rois (:130-162) and sample_bg_inds (:164-192) on the counts
    int n_fg = 0, bg_this = 0;
    bool fg_with_replacement = false, none = false;
    if (fg_num > 0 && bg_num > 0) {
        n_fg = min(cfg.fg_per_image, fg_num);
        bg_this = R - n_fg;
    } else if (fg_num > 0) {
        n_fg = R;
        fg_with_replacement = true;
    } else if (bg_num > 0) {
        bg_this = R;
    } else {
        none = true;  // the reference raises; only NaN IoUs come here
    }
    int n_hard = 0;
    if (hard_num > 0 && easy_num > 0)
        n_hard = min((int)((double)bg_this * cfg.hard_bg_ratio), hard_num);  // int(bg * ratio) as Python evaluates it
    else if (hard_num > 0)
        n_hard = bg_this;
    n_fg = max(0, min(n_fg, R));
    n_hard = max(0, min(n_hard, R - n_fg));

    const uint64_t key_fg = stream_key(dr.seed, s, PURPOSE_FG), key_hard = stream_key(dr.seed, s, PURPOSE_HARD),
                   key_easy = stream_key(dr.seed, s, PURPOSE_EASY);
    const float two_pi = (float)(2 * M_PI), pi = (float)M_PI, half_pi = (float)(M_PI * 0.5), pi_15 = (float)(M_PI * 1.5);
    bool my_bad = false;

    for (int r = threadIdx.x; r < R; r += ROI_SAMPLE_THREADS) {
        const size_t o = (size_t)s * R + r;
        if (none) {
            for (int c = 0; c < 7; ++c) out.rois[o * 7 + c] = 0.f;
            for (int c = 0; c < 8; ++c) out.gt_of_rois_src[o * 8 + c] = out.gt_of_rois[o * 8 + c] = 0.f;
            out.gt_iou[o] = 0.f;
            out.roi_scores[o] = 0.f;
            out.roi_labels[o] = 0;
            out.reg_valid_mask[o] = 0;
            if (cfg.score_type == 0) ((int64_t*)out.rcnn_cls_labels)[o] = 0;
            else ((float*)out.rcnn_cls_labels)[o] = 0.f;
            if (out.sampled_inds) out.sampled_inds[o] = -1;
            continue;
        }
        // which list, which entry of it
        int which, n;
        long long e;
        if (r < n_fg) {
            which = 0;
            n = fg_num;
            if (dr.explicit_draws)
                e = fg_with_replacement ? (long long)floor(dr.fg_rand[o] * (double)fg_num) : (long long)dr.perm[(size_t)s * m + r];
            else
                e = fg_with_replacement ? draw_below(key_fg, (uint32_t)r, (uint32_t)fg_num)
                                        : keyed_bijection(key_fg, (uint32_t)fg_num, (uint32_t)r);
        } else if (r < n_fg + n_hard) {
            const int q = r - n_fg;
            which = 1;
            n = hard_num;
            e = dr.explicit_draws ? (long long)dr.hard_draw[(size_t)s * R + q] : draw_below(key_hard, (uint32_t)q, (uint32_t)hard_num);
        } else {
            const int q = r - n_fg - n_hard;
            which = 2;
            n = easy_num;
            e = dr.explicit_draws ? (long long)dr.easy_draw[(size_t)s * R + q] : draw_below(key_easy, (uint32_t)q, (uint32_t)easy_num);
        }
        if (e < 0 || e >= n) {  // a draw outside its list (explicit mode only): reported, never followed
            my_bad = true;
            e = 0;
        }
        const int i = n > 0 ? lists[which][e] : 0;
        const size_t src = (size_t)s * m + i;
        const float iou = ov[i];
        int g = gt_assignment[src];
        if (g < 0 || g >= max(t, 1)) {
            my_bad = true;
            g = 0;
        }
        float roi[7], gb[8];
#pragma unroll
        for (int c = 0; c < 7; ++c) roi[c] = rois[src * 7 + c];
        if (t > 0) {
            const float* row = gt + ((size_t)s * t + g) * cols;
#pragma unroll
            for (int c = 0; c < 7; ++c) gb[c] = row[c];
            gb[7] = row[cols - 1];
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) gb[c] = 0.f;
        }
#pragma unroll
        for (int c = 0; c < 7; ++c) out.rois[o * 7 + c] = roi[c];
#pragma unroll
        for (int c = 0; c < 8; ++c) out.gt_of_rois_src[o * 8 + c] = gb[c];
        out.gt_iou[o] = iou;
        out.roi_scores[o] = roi_scores[src];
        out.roi_labels[o] = roi_labels[src];
        if (out.sampled_inds) out.sampled_inds[o] = i;
        out.reg_valid_mask[o] = iou > cfg.reg_fg ? 1 : 0;
        if (cfg.score_type == 0) {  // 'cls' (:39-43)
            int64_t l = iou > cfg.cls_fg ? 1 : 0;
            if (iou > cfg.cls_bg && iou < cfg.cls_fg) l = -1;
            ((int64_t*)out.rcnn_cls_labels)[o] = l;
        } else {                    // 'roi_iou' (:44-53)
            const bool fg = iou > cfg.cls_fg, bg = iou < cfg.cls_bg;
            float l = fg ? 1.f : 0.f;
            if (!fg && !bg) l = (iou - cfg.cls_bg) / cfg.fg_minus_bg;
            ((float*)out.rcnn_cls_labels)[o] = l;
        }
        // the canonical transformation (roi_head_template.py:113-133)
        const float roi_ry = torch_mod(roi[6], two_pi);
        const float dx = gb[0] - roi[0], dy = gb[1] - roi[1], dz = gb[2] - roi[2];
        // rotate_points_along_z(angle = -roi_ry): cos(-a) = cos a, sin(-a) = -sin a; through double, rounded once
        const float ca = (float)cos((double)roi_ry), sa = -(float)sin((double)roi_ry);
        float h = torch_mod(gb[6] - roi_ry, two_pi);
        if (h > half_pi && h < pi_15) h = torch_mod(h + pi, two_pi);
        if (h > pi) h = h - two_pi;
        h = h < -half_pi ? -half_pi : (h > half_pi ? half_pi : h);
        float* can = out.gt_of_rois + o * 8;
        can[0] = dx * ca + dy * (-sa);
        can[1] = dx * sa + dy * ca;
        can[2] = dz;
        can[3] = gb[3];
        can[4] = gb[4];
        can[5] = gb[5];
        can[6] = h;
        can[7] = gb[7];
    }
    if (my_bad) bad = 1;  // every writer stores the same value
    __syncthreads();
    if (threadIdx.x == 0) out.status[s] = none ? 1 : (bad ? 2 : 0);
}

}  // namespace
}  // namespace pda

PDA_API int pda_roi_max_iou(const float* rois, const int64_t* roi_labels, const float* gt_boxes, int gt_cols, int by_class,
                            float* max_overlaps, int32_t* gt_assignment, int b, int m, int t, pda_stream_t stream) {
    PDA_REQUIRE(b >= 0 && m >= 0 && t >= 0, "pda_roi_max_iou: b=%d m=%d t=%d", b, m, t);
    PDA_REQUIRE(gt_cols >= 8, "pda_roi_max_iou: gt_cols=%d < 8", gt_cols);
    PDA_REQUIRE(b <= 65535, "pda_roi_max_iou: batch %d > 65535", b);
    PDA_REQUIRE(m <= pda::ROI_MAX_M, "pda_roi_max_iou: m=%d > %d", m, pda::ROI_MAX_M);
    if (b == 0 || m == 0) return PDA_OK;
    PDA_REQUIRE(rois && max_overlaps && gt_assignment, "pda_roi_max_iou: null pointer");
    PDA_REQUIRE(t == 0 || gt_boxes, "pda_roi_max_iou: null gt_boxes");
    PDA_REQUIRE(!by_class || roi_labels, "pda_roi_max_iou: null roi_labels");
    hipLaunchKernelGGL(pda::roi_max_iou_kernel, dim3(pda::divup(m, pda::ROI_IOU_WAVES), b), dim3(64 * pda::ROI_IOU_WAVES), 0,
                       (hipStream_t)stream, rois, roi_labels, gt_boxes, gt_cols, by_class ? 1 : 0, max_overlaps,
                       gt_assignment, m, t);
    return pda::check_launch("pda_roi_max_iou");
}

PDA_API int pda_roi_sample_targets(const float* rois, const float* roi_scores, const int64_t* roi_labels,
                                   const float* gt_boxes, int gt_cols, const float* max_overlaps,
                                   const int32_t* gt_assignment, int roi_per_image, int fg_per_image, double hard_bg_ratio,
                                   double reg_fg_thresh, double cls_fg_thresh, double cls_bg_thresh, double cls_bg_thresh_lo,
                                   int score_type, const int32_t* perm, const double* fg_rand, const int64_t* hard_draw,
                                   const int64_t* easy_draw, uint64_t seed, float* out_rois, float* gt_of_rois_src,
                                   float* gt_of_rois, float* gt_iou_of_rois, float* out_roi_scores, int64_t* out_roi_labels,
                                   int64_t* reg_valid_mask, void* rcnn_cls_labels, int32_t* sampled_inds, int32_t* status,
                                   int b, int m, int t, pda_stream_t stream) {
    PDA_REQUIRE(b >= 0 && m >= 0 && t >= 0, "pda_roi_sample_targets: b=%d m=%d t=%d", b, m, t);
    PDA_REQUIRE(gt_cols >= 8, "pda_roi_sample_targets: gt_cols=%d < 8", gt_cols);
    PDA_REQUIRE(roi_per_image > 0, "pda_roi_sample_targets: roi_per_image=%d <= 0", roi_per_image);
    PDA_REQUIRE(fg_per_image >= 0 && fg_per_image <= roi_per_image, "pda_roi_sample_targets: fg_per_image=%d outside 0..%d",
                fg_per_image, roi_per_image);
    PDA_REQUIRE(hard_bg_ratio >= 0.0 && hard_bg_ratio <= 1.0, "pda_roi_sample_targets: hard_bg_ratio=%g outside [0, 1]",
                hard_bg_ratio);
    PDA_REQUIRE(score_type == 0 || score_type == 1, "pda_roi_sample_targets: score_type=%d (0 'cls', 1 'roi_iou')", score_type);
    PDA_REQUIRE(b <= 65535, "pda_roi_sample_targets: batch %d > 65535", b);
    PDA_REQUIRE(m <= pda::ROI_MAX_M, "pda_roi_sample_targets: m=%d > %d", m, pda::ROI_MAX_M);
    if (b == 0 || m == 0) return PDA_OK;
    PDA_REQUIRE(rois && roi_scores && roi_labels && max_overlaps && gt_assignment, "pda_roi_sample_targets: null input pointer");
    PDA_REQUIRE(t == 0 || gt_boxes, "pda_roi_sample_targets: null gt_boxes");
    PDA_REQUIRE(out_rois && gt_of_rois_src && gt_of_rois && gt_iou_of_rois && out_roi_scores && out_roi_labels &&
                    reg_valid_mask && rcnn_cls_labels && status,
                "pda_roi_sample_targets: null output pointer");
    const bool all = perm && fg_rand && hard_draw && easy_draw, any = perm || fg_rand || hard_draw || easy_draw;
    PDA_REQUIRE(all || !any, "pda_roi_sample_targets: explicit draws need perm, fg_rand, hard_draw and easy_draw");
    pda::RoiSampler cfg{};
    cfg.roi_per_image = roi_per_image;
    cfg.fg_per_image = fg_per_image;
    cfg.score_type = score_type;
    cfg.hard_bg_ratio = hard_bg_ratio;
    cfg.reg_fg = (float)reg_fg_thresh;
    cfg.cls_fg = (float)cls_fg_thresh;
    cfg.cls_bg = (float)cls_bg_thresh;
    cfg.cls_bg_lo = (float)cls_bg_thresh_lo;
    cfg.fg_thresh = (float)(reg_fg_thresh < cls_fg_thresh ? reg_fg_thresh : cls_fg_thresh);
    cfg.fg_minus_bg = (float)(cls_fg_thresh - cls_bg_thresh);
    pda::RoiDraws dr{perm, fg_rand, hard_draw, easy_draw, (unsigned long long)seed, all ? 1 : 0};
    pda::RoiTargetsOut out{out_rois,       gt_of_rois_src, gt_of_rois,      gt_iou_of_rois, out_roi_scores,
                           out_roi_labels, reg_valid_mask, rcnn_cls_labels, sampled_inds,   status};
    hipLaunchKernelGGL(pda::roi_sample_targets_kernel, dim3(b), dim3(pda::ROI_SAMPLE_THREADS), 0, (hipStream_t)stream, rois,
                       roi_scores, roi_labels, gt_boxes, gt_cols, max_overlaps, gt_assignment, cfg, dr, out, m, t);
    return pda::check_launch("pda_roi_sample_targets");
}
