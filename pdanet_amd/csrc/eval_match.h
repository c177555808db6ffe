// eval_match.h -- the matching core that the ONCE and KITTI evaluations share (once_eval.hip, kitti_eval.hip): the wave
// helpers, the frame record with its bounds-checked loader, the two greedy walks over a frame's GT rows, and the host
// check of the frame limits.  Both references state the same matching rule (ONCE accumulate_scores / compute_statistics,
// KITTI compute_statistics_jit with compute_fp False / True); what differs comes in as a parameter: where a GT's flag is
// read from, the score floor of the first pass, and what happens per true positive in the second (KITTI's AOS sum).
//
// Detections j of a frame are owned by lane j % 64 at bit j / 64 of 64-bit lane masks (accepted, ignored, assigned),
// hence EVAL_MAX_DET.  One wave runs a walk; the GT loop stays serial, as in the references.
//
// The 32-bit wave minimum is pda::wave_min_u32 of pda_common.h (DPP), not a copy of the shuffle loop: a minimum is exact,
// so the value is the same, it is one definition fewer, and it timed no slower (on 3769 KITTI-val-sized frames 13.0 ms
// of device time against 14.1 ms with the shuffle loop here; ONCE 15.3 ms either way).
//
// Left alone on purpose: once_thresh_kernel and kitti_thresh_kernel look alike but state different float64 arithmetic
// (s < 2 * level with an epsilon do-while that can append several thresholds per rank, against
// (r - level) < (level - l) with one append), each in its reference's operation order; the overlap kernels,
// kitti_flags_kernel, kitti_sim_kernel, kitti_pred_kernel, rotated_inter.h, bev_overlap.h and recall.hip share nothing
// with the matching.  Include after pda_common.h, inside no namespace.
#pragma once

#include <math.h>

namespace pda {

constexpr int EVAL_MAX_DET = 64 * 64;

// ---- wave helpers ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// float32 -> unsigned key with the order of the floats
__device__ __forceinline__ uint32_t ordered(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// bit j of the lane masks, wave-uniform
__device__ __forceinline__ bool lane_bit(uint64_t mask, int j) {
    return (__ballot((mask >> (j >> 6)) & 1ull) >> (j & 63)) & 1ull;
}

// ---- frame bookkeeping ----------------------------------------------------------------------------------------------
struct EvalFrame {
    int64_t g0, d0, o0;  // first GT row, first detection row, first overlap element
    int ng, nd, mode;    // mode: KITTI's frame_mode bits, 0 for ONCE
};

// The ranges of frame f, or an empty frame (status bit 1) when they leave the declared bounds.  frame_mode may be null.
__device__ __forceinline__ EvalFrame load_eval_frame(const int64_t* gt_offsets, const int64_t* det_start,
                                                     const int32_t* det_count, const int64_t* ov_start,
                                                     const int32_t* frame_mode, int max_gt, int max_det,
                                                     int64_t n_gt_total, int64_t det_cap, int64_t ov_cap, int f,
                                                     int32_t* status) {
    EvalFrame F;
    F.g0 = gt_offsets[f];
    const int64_t ng = gt_offsets[f + 1] - F.g0;
    F.d0 = det_start[f];
    const int64_t nd = det_count[f];
    F.o0 = ov_start[f];
    F.mode = frame_mode ? frame_mode[f] : 0;
    const bool ok = F.g0 >= 0 && ng >= 0 && ng <= max_gt && F.g0 + ng <= n_gt_total && nd >= 0 && nd <= max_det &&
                    F.d0 >= 0 && F.d0 + nd <= det_cap && F.o0 >= 0 && F.o0 + ng * nd <= ov_cap;
    if (!ok) {
        if (threadIdx.x == 0 && status) atomicOr(status, 1);
        F.g0 = F.d0 = F.o0 = 0;
        F.ng = F.nd = 0;
        return F;
    }
    F.ng = (int)ng;
    F.nd = (int)nd;
    return F;
}

// ---- the two walks --------------------------------------------------------------------------------------------------
// The score floors of the first pass, each as its reference writes it.
struct ScoreFloorOnce {  // accumulate_scores: max_score = -1 against the float32 scores
    static __device__ __forceinline__ bool above(float s) { return s > -1.0f; }
};
struct ScoreFloorKitti {  // compute_statistics_jit: valid_detection = NO_DETECTION = -10000000 in float64
    static __device__ __forceinline__ bool above(float s) { return (double)s > -10000000.0; }
};

// First pass over one frame: each GT i with gt_flag(i) != -1, in order, takes the highest-scoring unassigned accepted
// detection (first index on ties) with overlap > thr and a score over the floor; a pair with a flag of 1 on either side
// is only assigned, the others are true positives.  rows is the frame's ng x nd overlap block, score the frame's nd
// scores; acc / ign are the lane's masks (flag != -1, flag == 1).  Writes the TP scores and then -INFINITY up to ng into
// out; returns their number.
template <typename Floor, typename GtFlag>
__device__ __forceinline__ int match_first_pass(const double* rows, int ng, int nd, const float* __restrict__ score,
                                                uint64_t acc, uint64_t ign, double thr, GtFlag gt_flag,
                                                float* __restrict__ out) {
    const int lane = lane_id();
    uint64_t assigned = 0;
    int n_tp = 0;
    for (int i = 0; i < ng; ++i) {
        const int gf = gt_flag(i);
        if (gf == -1) continue;
        const double* row = rows + i * nd;
        uint64_t best = 0;
        for (uint64_t m = acc & ~assigned; m; m &= m - 1) {
            const int j = lane + 64 * (int)__builtin_ctzll(m);
            const float s = score[j];
            if (row[j] > thr && Floor::above(s)) {
                const uint64_t key = ((uint64_t)ordered(s) << 32) | (uint32_t)(0xffffffffu - (uint32_t)j);
                best = key > best ? key : best;
            }
        }
        best = wave_max_u64(best);
        if (best == 0) continue;
        const int jd = (int)(0xffffffffu - (uint32_t)best);
        if (lane == (jd & 63)) assigned |= 1ull << (jd >> 6);
        if (gf == 1 || lane_bit(ign, jd)) continue;
        if (lane == 0) out[n_tp] = score[jd];
        ++n_tp;
    }
    for (int s = n_tp + lane; s < ng; s += 64) out[s] = -INFINITY;
    return n_tp;
}

struct MatchStats {
    int tp, fn;
    uint64_t open;  // the lane's unmatched detections that count: acc & ~ign & above & ~assigned
};

// Second pass over one frame at score threshold th: among the accepted detections with a score not below th, each GT
// not flagged -1, in order, takes the unassigned one of the largest overlap > thr among flag 0 (first index on ties),
// else the first of flag 1; none is a false negative when the GT's flag is 0.  A flag-0 GT with a flag-0 detection is
// a true positive, and on_tp(i, j) is called for it, in GT order.
template <typename GtFlag, typename OnTp>
__device__ __forceinline__ MatchStats match_second_pass(const double* rows, int ng, int nd,
                                                        const float* __restrict__ score, uint64_t acc, uint64_t ign,
                                                        double thr, double th, GtFlag gt_flag, OnTp on_tp) {
    const int lane = lane_id();
    uint64_t above = 0;
    for (uint64_t m = acc; m; m &= m - 1) {
        const int k = (int)__builtin_ctzll(m);
        if (!((double)score[lane + 64 * k] < th)) above |= 1ull << k;
    }
    uint64_t assigned = 0;
    MatchStats r = {0, 0, 0};
    for (int i = 0; i < ng; ++i) {
        const int gf = gt_flag(i);
        if (gf == -1) continue;
        const double* row = rows + i * nd;
        uint64_t best0 = 0;  // overlap bits (positive doubles order as integers)
        uint32_t j0 = 0xffffffffu, j1 = 0xffffffffu;
        for (uint64_t m = acc & above & ~assigned; m; m &= m - 1) {
            const int k = (int)__builtin_ctzll(m);
            const int j = lane + 64 * k;
            const double v = row[j];
            if (!(v > thr)) continue;
            if ((ign >> k) & 1ull) {
                if ((uint32_t)j < j1) j1 = (uint32_t)j;
            } else {
                const uint64_t bits = (uint64_t)__double_as_longlong(v);
                if (bits > best0) { best0 = bits; j0 = (uint32_t)j; }
            }
        }
        const uint64_t m0 = wave_max_u64(best0);
        int jd;
        bool det_ign;
        if (m0 != 0) {
            jd = (int)wave_min_u32(best0 == m0 ? j0 : 0xffffffffu);
            det_ign = false;
        } else {
            const uint32_t w1 = wave_min_u32(j1);
            if (w1 == 0xffffffffu) {
                r.fn += gf == 0;
                continue;
            }
            jd = (int)w1;
            det_ign = true;
        }
        if (lane == (jd & 63)) assigned |= 1ull << (jd >> 6);
        if (gf == 1 || det_ign) continue;
        ++r.tp;
        on_tp(i, jd);
    }
    r.open = acc & ~ign & above & ~assigned;
    return r;
}

// ---- host side ------------------------------------------------------------------------------------------------------
// The size limits of a frame set; det_word is the caller's name of its detection bound ("max_pred", "max_det").
inline int check_frame_limits(const char* what, const char* det_word, int n_frames, int max_gt, int max_det,
                              int64_t n_gt_total, int64_t det_cap, int64_t ov_cap) {
    PDA_REQUIRE(n_frames >= 0 && n_frames <= (1 << 24), "%s: n_frames %d outside [0, 2^24]", what, n_frames);
    PDA_REQUIRE(max_gt >= 0 && max_det >= 0 && max_det <= EVAL_MAX_DET, "%s: max_gt %d / %s %d (%s <= %d)", what,
                max_gt, det_word, max_det, det_word, EVAL_MAX_DET);
    PDA_REQUIRE(n_gt_total >= 0 && det_cap >= 0 && ov_cap >= 0, "%s: negative sizes", what);
    PDA_REQUIRE((int64_t)max_gt * max_det <= ((int64_t)65535 * 256), "%s: max_gt x %s too large", what, det_word);
    return PDA_OK;
}

}  // namespace pda
