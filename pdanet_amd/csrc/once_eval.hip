// once_eval.hip -- ONCE detection evaluation on the device: the reference's once_eval get_evaluation_results
// (evaluation.py, eval_utils.py, iou_utils.py) minus the final float64 AP composition, which the caller does on the
// (tasks, thresholds, 3) counts.
//
//   once_iou_kernel     one thread per (frame, GT, prediction) pair: iou3d_kernel(_with_heading) of the frame's block.
//   once_accum_kernel   one wave per (frame, class, level): accumulate_scores; TP scores into the task's segment.
//   once_thresh_kernel  one wave per (class, level): get_thresholds over the descending TP scores.
//   once_stats_kernel   four waves per (frame, class, level), one threshold each in turn: compute_statistics, summed
//                       with integer atomics (order-independent, so deterministic).
//
// The frame record, the lane masks over predictions (hence max_pred <= 4096) and the two greedy walks over a frame's GT
// rows are eval_match.h, shared with kitti_eval.hip; here are ONCE's flags, its score floor and its thresholds.
#include "pda_common.h"
#include "rotated_inter.h"
#include "eval_match.h"

#include <math.h>

namespace pda {
namespace {

constexpr int OE_MAX_CLASSES = 16;
constexpr int OE_MAX_NAMES = 64;

struct EvalArgs {
    uint64_t accept[OE_MAX_CLASSES];  // bit n: the class takes name id n
    double thr[OE_MAX_CLASSES];
    int n_classes, n_names, n_levels, mode;
};

// ---- rotated BEV intersection, iou_utils.py (numba.cuda) -------------------------------------------------------------
// rotated_inter.h with ONCE's point test (the edge cross-product signs); rotate_iou_kernel_eval stores the float64 area
// as float32.

// devRotateIoUEval(rbox1 = pred, rbox2 = gt, criterion = 2): the intersection area, rounded to float32.
__device__ float rotated_intersection(const float* q, const float* g) {
    return (float)rotated_intersection_area<InQuadCross>(q, g);
}

// ---- frame bookkeeping --------------------------------------------------------------------------------------------
__device__ __forceinline__ EvalFrame load_frame(const pda_once_frames_t& fr, int f, int32_t* status) {
    return load_eval_frame(fr.gt_offsets, fr.pred_start, fr.pred_count, fr.iou_start, nullptr, fr.max_gt, fr.max_pred,
                           fr.n_gt_total, fr.pred_cap, fr.iou_cap, f, status);
}

// overall_distance_filter / distance_filter / overall_filter: true = the box is in the level (flag not 1).  The norm
// follows np.sqrt(np.sum(b[:, 0:3] * b[:, 0:3], axis=1)) in the boxes' dtype: float64 for GT, float32 for predictions.
template <typename T> __device__ __forceinline__ bool in_level(T x, T y, T z, int mode, int level) {
    if (mode == 1) return true;
    if (mode == 0) {
        if (level == 0) return true;
        --level;
    }
    const T d = sqrt((x * x + y * y) + z * z);
    if (level == 0) return d < T(30);
    if (level == 1) return d >= T(30) && d < T(50);
    return d >= T(50);
}

// filter_data: the class rejection (-1) is written first and the level's ignore (1) over it, so a box of another class
// outside the level is flagged 1, as in the reference.
__device__ __forceinline__ int name_ok(const EvalArgs& a, int cls, int name, int32_t* status) {
    if (name < 0 || name >= a.n_names) {
        if (status) atomicOr(status, 2);
        return 0;
    }
    return (int)((a.accept[cls] >> name) & 1ull);
}

__device__ __forceinline__ int gt_flag(const pda_once_frames_t& fr, const EvalArgs& a, int64_t row, int cls, int level) {
    const double* b = fr.gt_boxes + row * 7;
    if (!in_level<double>(b[0], b[1], b[2], a.mode, level)) return 1;
    return name_ok(a, cls, fr.gt_name[row], nullptr) ? 0 : -1;
}

// The lane's prediction masks for (cls, level): bit k <-> prediction lane + 64 k.  acc: flag != -1, ign: flag == 1.
__device__ __forceinline__ void pred_masks(const pda_once_frames_t& fr, const EvalArgs& a, const EvalFrame& F, int cls,
                                           int level, int32_t* status, uint64_t& acc, uint64_t& ign) {
    acc = ign = 0;
    const int lane = lane_id();
    for (int j = lane, k = 0; j < F.nd; j += 64, ++k) {
        const int64_t row = F.d0 + j;
        const float* b = fr.pred_boxes + row * 7;
        const bool lev = in_level<float>(b[0], b[1], b[2], a.mode, level);
        const int ok = name_ok(a, cls, fr.pred_name[row], status);
        if (!lev) { acc |= 1ull << k; ign |= 1ull << k; }
        else if (ok) acc |= 1ull << k;
    }
}

// ---- kernels ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) once_iou_kernel(pda_once_frames_t fr, int with_heading, double* __restrict__ iou,
                                                       int32_t* status) {
    const int f = blockIdx.x;
    const EvalFrame F = load_frame(fr, f, status);
    const int64_t pair = (int64_t)blockIdx.y * blockDim.x + threadIdx.x;
    if (pair >= (int64_t)F.ng * F.nd) return;
    const int i = (int)(pair / F.nd), j = (int)(pair % F.nd);
    const double* g = fr.gt_boxes + (F.g0 + i) * 7;
    const float* p = fr.pred_boxes + (F.d0 + j) * 7;
    // rotate_iou_gpu_eval casts both box sets to float32 and returns the float32 areas in the GT dtype
    const float g5[5] = {(float)g[0], (float)g[1], (float)g[3], (float)g[4], (float)g[6]};
    const float p5[5] = {p[0], p[1], p[3], p[4], p[6]};
    const double inter2d = (double)rotated_intersection(p5, g5);
    // heights and volumes: numpy arithmetic in each side's dtype, float64 once the two meet
    const double g_max = g[2] + g[5] * 0.5, g_min = g[2] - g[5] * 0.5;
    const float p_max = p[2] + p[5] * 0.5f, p_min = p[2] - p[5] * 0.5f;
    const double max_of_min = fmax(g_min, (double)p_min), min_of_max = fmin(g_max, (double)p_max);
    double inter_h = min_of_max - max_of_min;
    if (inter_h <= 0) inter_h = 0;
    const double inter3d = inter2d * inter_h;
    const double g_vol = g[3] * g[4] * g[5];
    const float p_vol = p[3] * p[4] * p[5];
    const double uni = (g_vol + (double)p_vol) - inter3d;
    double v = inter3d / uni;
    if (with_heading) {
        double dr = fabs(g[6] - (double)p[6]);
        if (dr >= M_PI) dr = 2 * M_PI - dr;
        if (dr > M_PI / 2) v = 0;
    }
    iou[F.o0 + pair] = v;
}

// accumulate_scores of one (frame, class, level); blockIdx.y = task = class * n_levels + level.
__global__ void __launch_bounds__(64) once_accum_kernel(pda_once_frames_t fr, const double* __restrict__ iou, EvalArgs a,
                                                        float* __restrict__ seg, int64_t* ntp, int64_t* nvalid,
                                                        int32_t* status) {
    const int f = blockIdx.x, task = blockIdx.y, cls = task / a.n_levels, level = task % a.n_levels;
    const int lane = lane_id();
    const EvalFrame F = load_frame(fr, f, status);
    uint64_t acc, ign;
    pred_masks(fr, a, F, cls, level, status, acc, ign);
    int n_valid = 0;
    const auto flag = [&](int i) {
        const int gf = gt_flag(fr, a, F.g0 + i, cls, level);
        n_valid += gf == 0;
        return gf;
    };
    const int n_tp = match_first_pass<ScoreFloorOnce>(iou + F.o0, F.ng, F.nd, fr.pred_score + F.d0, acc, ign, a.thr[cls],
                                                      flag, seg + (int64_t)task * fr.n_gt_total + F.g0);
    if (lane == 0) {
        atomicAdd((unsigned long long*)&ntp[task], (unsigned long long)n_tp);
        atomicAdd((unsigned long long*)&nvalid[task], (unsigned long long)n_valid);
    }
}

// get_thresholds of one task over its n TP scores, sorted descending; float64 throughout, recall_level advanced by
// repeated += 1 / num_pr_points.  r + l is non-decreasing in i, so a wave evaluates 64 ranks at a time and the serial
// walk only visits the ranks that append.
__global__ void __launch_bounds__(64) once_thresh_kernel(const float* __restrict__ sorted, int64_t n_gt_total,
                                                         const int64_t* ntp, const int64_t* nvalid, int num_pr_points,
                                                         double* thresholds, int64_t* n_thr, int32_t* status) {
    const int task = blockIdx.x, lane = lane_id();
    const int64_t n = ntp[task];
    const double g = (double)nvalid[task];
    const float* sc = sorted + (int64_t)task * n_gt_total;
    double* out = thresholds + (int64_t)task * (num_pr_points + 1);
    const double eps = 1e-6, inc = 1.0 / (double)num_pr_points;
    double level = 0.0;
    int64_t nt = 0;
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t i = base + lane;
        const double l = (double)(i + 1) / g;
        const double r = i < n - 1 ? (double)(i + 2) / g : l;
        const double s = r + l;
        int64_t cursor = base;
        while (true) {
            const uint64_t take = __ballot(i < n && i >= cursor && !(s < 2 * level && i < n - 1));
            if (!take) break;
            const int p = (int)__builtin_ctzll(take);
            const double sp = __shfl(s, p, 64);
            const double v = (double)sc[base + p];
            do {
                if (lane == 0 && nt <= num_pr_points) out[nt] = v;
                ++nt;
                level += inc;
            } while (sp + eps > 2 * level);
            cursor = base + p + 1;
        }
    }
    if (lane == 0) {
        n_thr[task] = nt;
        if (nt > num_pr_points + 1) atomicOr(status, 4);
    }
}

// compute_statistics of one (frame, task) for thresholds t = wave, wave + 4, ...  With iou_thr >= 0 the reference's
// per-GT state machine picks the first prediction of the highest IoU among the level's predictions (flag 0), else the
// first ignored one (flag 1).
__global__ void __launch_bounds__(256) once_stats_kernel(pda_once_frames_t fr, const double* __restrict__ iou, EvalArgs a,
                                                         int num_pr_points, const double* __restrict__ thresholds,
                                                         const int64_t* __restrict__ n_thr, int64_t* counts,
                                                         int32_t* status) {
    const int f = blockIdx.x, task = blockIdx.y, cls = task / a.n_levels, level = task % a.n_levels;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const EvalFrame F = load_frame(fr, f, status);
    uint64_t acc, ign;
    pred_masks(fr, a, F, cls, level, nullptr, acc, ign);
    const double thr = a.thr[cls];
    const auto flag = [&](int i) { return gt_flag(fr, a, F.g0 + i, cls, level); };
    int64_t nt = n_thr[task];
    if (nt > num_pr_points + 1) nt = num_pr_points + 1;
    for (int t = wave; t < nt; t += 4) {
        const double th = thresholds[(int64_t)task * (num_pr_points + 1) + t];
        const MatchStats r = match_second_pass(iou + F.o0, F.ng, F.nd, fr.pred_score + F.d0, acc, ign, thr, th, flag,
                                               [](int, int) {});
        const int tp = r.tp, fn = r.fn, fp = wave_sum_i32(__builtin_popcountll(r.open));
        if (lane == 0) {
            int64_t* c = counts + ((int64_t)task * (num_pr_points + 1) + t) * 3;
            if (tp) atomicAdd((unsigned long long*)&c[0], (unsigned long long)tp);
            if (fp) atomicAdd((unsigned long long*)&c[1], (unsigned long long)fp);
            if (fn) atomicAdd((unsigned long long*)&c[2], (unsigned long long)fn);
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
int64_t seg_bytes(int64_t n_gt_total, int n_tasks) { return (n_tasks * n_gt_total * 4 + 255) / 256 * 256; }

int check_frames(const pda_once_frames_t* fr, const char* what) {
    PDA_REQUIRE(fr, "%s: null frames", what);
    if (int st = check_frame_limits(what, "max_pred", fr->n_frames, fr->max_gt, fr->max_pred, fr->n_gt_total, fr->pred_cap,
                                    fr->iou_cap))
        return st;
    if (fr->n_frames == 0) return PDA_OK;
    PDA_REQUIRE(fr->gt_offsets && fr->pred_start && fr->pred_count && fr->iou_start, "%s: null frame arrays", what);
    PDA_REQUIRE((fr->gt_boxes && fr->gt_name) || fr->n_gt_total == 0, "%s: null GT arrays", what);
    PDA_REQUIRE((fr->pred_boxes && fr->pred_score && fr->pred_name) || fr->pred_cap == 0, "%s: null prediction arrays",
                what);
    return PDA_OK;
}

int make_args(EvalArgs& a, const uint8_t* accept, int n_classes, int n_names, const double* iou_thr, int mode,
              const char* what) {
    PDA_REQUIRE(n_classes >= 1 && n_classes <= OE_MAX_CLASSES, "%s: n_classes %d outside [1, %d]", what, n_classes,
                OE_MAX_CLASSES);
    PDA_REQUIRE(n_names >= 1 && n_names <= OE_MAX_NAMES, "%s: n_names %d outside [1, %d]", what, n_names, OE_MAX_NAMES);
    PDA_REQUIRE(mode >= 0 && mode <= 2, "%s: difficulty_mode %d outside [0, 2]", what, mode);
    PDA_REQUIRE(accept && iou_thr, "%s: null accept table or thresholds", what);
    a = EvalArgs{};
    for (int c = 0; c < n_classes; ++c) {
        PDA_REQUIRE(iou_thr[c] >= 0.0, "%s: iou threshold %g of class %d < 0", what, iou_thr[c], c);
        a.thr[c] = iou_thr[c];
        for (int n = 0; n < n_names; ++n)
            if (accept[c * n_names + n]) a.accept[c] |= 1ull << n;
    }
    a.n_classes = n_classes;
    a.n_names = n_names;
    a.mode = mode;
    a.n_levels = mode == 0 ? 4 : mode == 1 ? 1 : 3;
    return PDA_OK;
}

}  // namespace
}  // namespace pda

PDA_API int64_t pda_once_eval_workspace_bytes(int n_frames, int64_t n_gt_total, int n_tasks) {
    if (n_frames < 0 || n_gt_total < 0 || n_gt_total > ((int64_t)1 << 31) || n_tasks < 1 ||
        n_tasks > pda::OE_MAX_CLASSES * 4)
        return -1;
    return pda::seg_bytes(n_gt_total, n_tasks) + (int64_t)n_tasks * 8;
}

PDA_API int pda_once_eval_iou(const pda_once_frames_t* fr, int with_heading, double* iou, int32_t* status,
                              pda_stream_t stream) {
    if (int st = pda::check_frames(fr, "pda_once_eval_iou")) return st;
    PDA_REQUIRE(status, "pda_once_eval_iou: null status");
    if (fr->n_frames == 0) return PDA_OK;
    PDA_REQUIRE(iou || fr->iou_cap == 0, "pda_once_eval_iou: null iou");
    const int64_t pairs = (int64_t)fr->max_gt * fr->max_pred;
    if (pairs == 0) return PDA_OK;
    hipLaunchKernelGGL(pda::once_iou_kernel, dim3((unsigned)fr->n_frames, (unsigned)pda::divup64(pairs, 256)), dim3(256), 0,
                       (hipStream_t)stream, *fr, with_heading ? 1 : 0, iou, status);
    return pda::check_launch("pda_once_eval_iou");
}

PDA_API int pda_once_eval_accumulate(const pda_once_frames_t* fr, const double* iou, const uint8_t* accept, int n_classes,
                                     int n_names, const double* iou_thr, int difficulty_mode, int64_t* num_valid_gt,
                                     int32_t* status, void* workspace, pda_stream_t stream) {
    const char* what = "pda_once_eval_accumulate";
    if (int st = pda::check_frames(fr, what)) return st;
    pda::EvalArgs a;
    if (int st = pda::make_args(a, accept, n_classes, n_names, iou_thr, difficulty_mode, what)) return st;
    const int n_tasks = n_classes * a.n_levels;
    PDA_REQUIRE(pda_once_eval_workspace_bytes(fr->n_frames, fr->n_gt_total, n_tasks) >= 0, "%s: bad sizes", what);
    PDA_REQUIRE(workspace && num_valid_gt && status, "%s: null workspace, num_valid_gt or status", what);
    PDA_REQUIRE(iou || fr->iou_cap == 0, "%s: null iou", what);
    hipStream_t st = (hipStream_t)stream;
    float* seg = (float*)workspace;
    int64_t* ntp = (int64_t*)((char*)workspace + pda::seg_bytes(fr->n_gt_total, n_tasks));
    if (hipMemsetAsync(ntp, 0, n_tasks * 8, st) != hipSuccess || hipMemsetAsync(num_valid_gt, 0, n_tasks * 8, st) != hipSuccess)
        return pda::check_launch(what);
    if (fr->n_frames == 0) return PDA_OK;
    hipLaunchKernelGGL(pda::once_accum_kernel, dim3((unsigned)fr->n_frames, (unsigned)n_tasks), dim3(64), 0, st, *fr, iou, a,
                       seg, ntp, num_valid_gt, status);
    return pda::check_launch(what);
}

PDA_API int pda_once_eval_match(const pda_once_frames_t* fr, const double* iou, const uint8_t* accept, int n_classes,
                                int n_names, const double* iou_thr, int difficulty_mode, int num_pr_points,
                                const float* sorted_scores, const int64_t* num_valid_gt, double* thresholds,
                                int64_t* n_thresholds, int64_t* counts, int32_t* status, void* workspace,
                                pda_stream_t stream) {
    const char* what = "pda_once_eval_match";
    if (int st = pda::check_frames(fr, what)) return st;
    pda::EvalArgs a;
    if (int st = pda::make_args(a, accept, n_classes, n_names, iou_thr, difficulty_mode, what)) return st;
    PDA_REQUIRE(num_pr_points >= 1 && num_pr_points <= 100000, "%s: num_pr_points %d outside [1, 100000]", what,
                num_pr_points);
    const int n_tasks = n_classes * a.n_levels;
    PDA_REQUIRE(pda_once_eval_workspace_bytes(fr->n_frames, fr->n_gt_total, n_tasks) >= 0, "%s: bad sizes", what);
    PDA_REQUIRE(workspace && num_valid_gt && thresholds && n_thresholds && counts && status,
                "%s: null workspace or output", what);
    PDA_REQUIRE(sorted_scores || fr->n_gt_total == 0, "%s: null sorted_scores", what);
    PDA_REQUIRE(iou || fr->iou_cap == 0, "%s: null iou", what);
    hipStream_t st = (hipStream_t)stream;
    const int64_t* ntp = (const int64_t*)((const char*)workspace + pda::seg_bytes(fr->n_gt_total, n_tasks));
    const int64_t n_counts = (int64_t)n_tasks * (num_pr_points + 1) * 3;
    if (hipMemsetAsync(counts, 0, n_counts * 8, st) != hipSuccess) return pda::check_launch(what);
    hipLaunchKernelGGL(pda::once_thresh_kernel, dim3((unsigned)n_tasks), dim3(64), 0, st, sorted_scores, fr->n_gt_total, ntp,
                       num_valid_gt, num_pr_points, thresholds, n_thresholds, status);
    if (fr->n_frames > 0)
        hipLaunchKernelGGL(pda::once_stats_kernel, dim3((unsigned)fr->n_frames, (unsigned)n_tasks), dim3(256), 0, st, *fr,
                           iou, a, num_pr_points, thresholds, n_thresholds, counts, status);
    return pda::check_launch(what);
}
