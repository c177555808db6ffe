// kitti_eval.hip -- KITTI detection evaluation on the device: the reference's kitti_object_eval_python eval.py
// get_official_eval_result (image / BEV / 3D / AOS, both R11 and R40) minus the final float64 composition, which the
// caller does on the read-back (tasks, 41, tp / fp / fn / similarity) table; and generate_prediction_dicts' lidar ->
// camera -> image conversion.
//
//   kitti_overlap_kernel   one thread per (frame, GT, detection) pair: image_box_overlap, the BEV rotate_iou and the 3D
//                          d3_box_overlap of the frame's block (calculate_iou_partly(dt_annos, gt_annos) only uses it).
//   kitti_flags_kernel     one block per frame: clean_data's ignored_gt / ignored_det for every (class, difficulty),
//                          num_valid_gt, and each detection's largest DontCare overlap (criterion 0).
//   kitti_pass1_kernel     one block per (frame, metric), one wave per (class, difficulty, overlap setting) in turn:
//                          compute_statistics_jit(compute_fp=False); TP scores into the task's segment.
//   kitti_thresh_kernel    one wave per task: get_thresholds over the descending TP scores (41 sample points).
//   kitti_pass2_kernel     one block per (frame, metric), one wave per (task, threshold) in turn: compute_statistics_jit
//                          (compute_fp=True); tp / fp / fn summed with integer atomics, the AOS similarity stored per
//                          frame.
//   kitti_sim_kernel       one thread per (metric-0 task, threshold): the frame similarities summed in frame order.
//   kitti_pred_kernel      one thread per prediction: boxes3d_lidar_to_kitti_camera, the image box, alpha.
//
// The pass kernels keep the frame's overlap block of their metric in LDS across every task and threshold when it fits
// (KE_LDS_DOUBLES); otherwise they read it from global memory.  The frame record, the lane masks over detections (hence
// max_det <= 4096) and the two greedy walks over a frame's GT rows are eval_match.h, shared with once_eval.hip.
#include "pda_common.h"
#include "rotated_inter.h"
#include "eval_match.h"

#include <math.h>

namespace pda {
namespace {

constexpr int KE_MAX_CLASSES = 6;
constexpr int KE_MAX_NAMES = 64;
constexpr int KE_NS = 41;              // N_SAMPLE_PTS
constexpr int KE_LDS_DOUBLES = 6144;   // 48 KiB
constexpr int KE_CALIB = 33;           // P2 (3 x 4), R0 (3 x 3), V2C (3 x 4)

// frame_mode bits: the dtypes numpy sees in the frame's part (get_split_parts(n, 100) of eval_class)
constexpr int KM_IMG_DT64 = 1;  // detection bboxes float64: image overlaps computed and stored as float64
constexpr int KM_IMG_GT64 = 2;  // GT bboxes float64
constexpr int KM_3D_DT64 = 4;   // detection location / dimensions / rotation_y float64
constexpr int KM_DC_DT64 = 8;   // detection bbox / alpha / score (dt_datas) float64

// clean_data's difficulty tables
__constant__ const double kMaxOcc[3] = {0, 1, 2};
__constant__ const double kMaxTrunc[3] = {0.15, 0.3, 0.5};
__constant__ const float kMinHeight[3] = {40, 25, 25};

struct KittiArgs {
    int8_t gt_class[KE_MAX_CLASSES][KE_MAX_NAMES];  // 1 the class, 0 its ignored neighbour (Van, Person_sitting), -1
    uint64_t dt_class[KE_MAX_CLASSES];               // bit n: a detection named n is of the class
    uint64_t dontcare;                               // bit n: name n is "DontCare"
    double min_overlap[2][3][KE_MAX_CLASSES];        // [setting][metric][class]
    int n_classes, n_names, compute_aos;
};

__device__ __forceinline__ EvalFrame load_kframe(const pda_kitti_frames_t& fr, int f, int32_t* status) {
    return load_eval_frame(fr.gt_offsets, fr.dt_start, fr.dt_count, fr.ov_start, fr.frame_mode, fr.max_gt, fr.max_det,
                           fr.n_gt_total, fr.det_cap, fr.ov_cap, f, status);
}

// numba's min / max of a float32 and a float64 unify to float64
template <typename T> __device__ __forceinline__ T mn(T a, T b) { return a < b ? a : b; }
template <typename T> __device__ __forceinline__ T mx(T a, T b) { return a > b ? a : b; }

// image_box_overlap(boxes, query_boxes, criterion) for one pair: each area in its own array's dtype, the rest in the
// common dtype, the result rounded to the boxes' dtype (overlaps = np.zeros(.., dtype=boxes.dtype)).
template <typename TB, typename TQ>
__device__ __forceinline__ double image_overlap(const float* bf, const TQ* q, int criterion) {
    using T = decltype(TB() + TQ());
    const TB b0 = bf[0], b1 = bf[1], b2 = bf[2], b3 = bf[3];
    const TQ qa = (q[2] - q[0]) * (q[3] - q[1]);
    const T iw = mn<T>(b2, q[2]) - mx<T>(b0, q[0]);
    if (!(iw > 0)) return 0.0;
    const T ih = mn<T>(b3, q[3]) - mx<T>(b1, q[1]);
    if (!(ih > 0)) return 0.0;
    const TB ba = (b2 - b0) * (b3 - b1);
    const T ua = criterion == -1 ? ((T)ba + (T)qa) - iw * ih : (T)ba;
    return (double)(TB)(iw * ih / ua);
}

// The lane's detection masks for (class, difficulty) cd: bit k <-> detection lane + 64 k.  acc: ignored_det != -1,
// ign: ignored_det == 1.
__device__ __forceinline__ void det_masks(const int8_t* __restrict__ dt_flags, const EvalFrame& F, uint64_t& acc,
                                          uint64_t& ign) {
    acc = ign = 0;
    for (int j = lane_id(), k = 0; j < F.nd; j += 64, ++k) {
        const int fl = dt_flags[F.d0 + j];
        if (fl != -1) acc |= 1ull << k;
        if (fl == 1) ign |= 1ull << k;
    }
}

// The frame's overlap block of one metric: into LDS when it fits, else the global block itself.
__device__ __forceinline__ const double* stage_block(const double* __restrict__ ov, const EvalFrame& F, double* lds) {
    const double* src = ov + F.o0;
    const int n = F.ng * F.nd;
    if (n > KE_LDS_DOUBLES) return src;
    for (int e = threadIdx.x; e < n; e += blockDim.x) lds[e] = src[e];
    __syncthreads();
    return lds;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------
// overlaps[m] at o0 + i * nd + j: metric m of GT i and detection j (the transpose of the reference's (dt x gt) block).
__global__ void __launch_bounds__(256) kitti_overlap_kernel(pda_kitti_frames_t fr, double* __restrict__ ov,
                                                            int32_t* status) {
    const int f = blockIdx.x;
    const EvalFrame F = load_kframe(fr, f, status);
    const int64_t pair = (int64_t)blockIdx.y * blockDim.x + threadIdx.x;
    if (pair >= (int64_t)F.ng * F.nd) return;
    const int i = (int)(pair / F.nd), j = (int)(pair % F.nd);
    const int64_t gr = F.g0 + i, dr = F.d0 + j;
    // metric 0: image_box_overlap(boxes = detections, query_boxes = GT, -1)
    const float* gb = fr.gt_bbox + gr * 4;
    const float* db = fr.dt_bbox + dr * 4;
    double v0;
    if (F.mode & KM_IMG_GT64) {
        const double q[4] = {gb[0], gb[1], gb[2], gb[3]};
        v0 = (F.mode & KM_IMG_DT64) ? image_overlap<double, double>(db, q, -1) : image_overlap<float, double>(db, q, -1);
    } else {
        v0 = (F.mode & KM_IMG_DT64) ? image_overlap<double, float>(db, gb, -1) : image_overlap<float, float>(db, gb, -1);
    }
    // metrics 1, 2: rotate_iou_gpu_eval(boxes = detections, query_boxes = GT) on (x, z, l, w, ry) cast to float32, i.e.
    // devRotateIoUEval(rbox1 = GT, rbox2 = detection)
    const float* gl = fr.gt_loc + gr * 3;
    const double* gd = fr.gt_dims + gr * 3;
    const float* dx = fr.dt_box + dr * 7;
    const float g5[5] = {gl[0], gl[2], (float)gd[0], (float)gd[2], (float)fr.gt_ry[gr]};
    const float d5[5] = {dx[0], dx[2], dx[3], dx[5], dx[6]};
    const double inter = rotated_intersection_area<InQuadProj>(g5, d5);
    const float area1 = g5[2] * g5[3], area2 = d5[2] * d5[3];
    const float bev = (float)(inter / ((double)(area1 + area2) - inter));
    // metric 2: rinc = the float32 BEV intersection; d3_box_overlap_kernel overwrites it in place with the 3D IoU, the
    // height overlap along camera -y
    float rinc = (float)inter;
    if (rinc > 0) {
        const double gy = gl[1], gh = gd[1];
        double iw, vol_d;
        if (F.mode & KM_3D_DT64) {
            const double y = dx[1], h = dx[4];
            iw = mn<double>(y, gy) - mx<double>(y - h, gy - gh);
            vol_d = ((double)dx[3] * (double)dx[4]) * (double)dx[5];
        } else {
            const float yh = dx[1] - dx[4];
            iw = mn<double>(dx[1], gy) - mx<double>(yh, gy - gh);
            vol_d = (double)((dx[3] * dx[4]) * dx[5]);
        }
        if (iw > 0) {
            const double vol_g = (gd[0] * gd[1]) * gd[2];
            const double inc = iw * (double)rinc;
            const double ua = (vol_d + vol_g) - inc;
            rinc = (float)(inc / ua);
        } else {
            rinc = 0.0f;
        }
    }
    const int64_t e = F.o0 + pair;
    ov[e] = v0;
    ov[fr.ov_cap + e] = (double)bev;
    ov[2 * fr.ov_cap + e] = (double)rinc;
}

// clean_data for every (class, difficulty) cd = class * 3 + difficulty; dc_max[row] = the largest
// image_box_overlap(detection, DontCare, criterion 0) of the detection's frame, -1 without DontCare.
__global__ void __launch_bounds__(256) kitti_flags_kernel(pda_kitti_frames_t fr, KittiArgs a, int8_t* __restrict__ gt_flags,
                                                          int8_t* __restrict__ dt_flags, double* __restrict__ dc_max,
                                                          int64_t* num_valid_gt, int32_t* status) {
    __shared__ int nvalid[KE_MAX_CLASSES * 3];
    const int f = blockIdx.x, ncd = a.n_classes * 3;
    const EvalFrame F = load_kframe(fr, f, status);
    if (threadIdx.x < ncd) nvalid[threadIdx.x] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < F.ng; i += blockDim.x) {
        const int64_t r = F.g0 + i;
        const int name = fr.gt_name[r];
        const bool name_ok = name >= 0 && name < a.n_names;
        if (!name_ok) atomicOr(status, 2);
        const float* b = fr.gt_bbox + r * 4;
        const float height = b[3] - b[1];
        const double occ = fr.gt_occ[r], trunc = fr.gt_trunc[r];
        for (int c = 0; c < a.n_classes; ++c) {
            const int vc = name_ok ? a.gt_class[c][name] : -1;
            for (int d = 0; d < 3; ++d) {
                const bool ignore = occ > kMaxOcc[d] || trunc > kMaxTrunc[d] || height <= kMinHeight[d];
                int fl = -1;
                if (vc == 1 && !ignore) {
                    fl = 0;
                    atomicAdd(&nvalid[c * 3 + d], 1);
                } else if (vc == 0 || (ignore && vc == 1)) {
                    fl = 1;
                }
                gt_flags[(int64_t)(c * 3 + d) * fr.n_gt_total + r] = (int8_t)fl;
            }
        }
    }
    for (int j = threadIdx.x; j < F.nd; j += blockDim.x) {
        const int64_t r = F.d0 + j;
        const int name = fr.dt_name[r];
        const bool name_ok = name >= 0 && name < a.n_names;
        if (!name_ok) atomicOr(status, 2);
        const float* b = fr.dt_bbox + r * 4;
        const float height = fabsf(b[3] - b[1]);
        for (int c = 0; c < a.n_classes; ++c) {
            const bool vc = name_ok && ((a.dt_class[c] >> name) & 1ull);
            for (int d = 0; d < 3; ++d) {
                const int fl = height < kMinHeight[d] ? 1 : vc ? 0 : -1;
                dt_flags[(int64_t)(c * 3 + d) * fr.det_cap + r] = (int8_t)fl;
            }
        }
        // overlaps_dt_dc = image_box_overlap(dt_bboxes, dc_bboxes (float64), 0)
        double m = -1.0;
        for (int i = 0; i < F.ng; ++i) {
            const int gn = fr.gt_name[F.g0 + i];
            if (gn < 0 || gn >= a.n_names || !((a.dontcare >> gn) & 1ull)) continue;
            const float* g = fr.gt_bbox + (F.g0 + i) * 4;
            const double q[4] = {g[0], g[1], g[2], g[3]};
            const double v = (F.mode & KM_DC_DT64) ? image_overlap<double, double>(b, q, 0) : image_overlap<float, double>(b, q, 0);
            m = v > m ? v : m;
        }
        dc_max[r] = m;
    }
    __syncthreads();
    if (threadIdx.x < ncd && nvalid[threadIdx.x])
        atomicAdd((unsigned long long*)&num_valid_gt[threadIdx.x], (unsigned long long)nvalid[threadIdx.x]);
}

// Task t = ((metric * n_classes + class) * 3 + difficulty) * 2 + setting; its (class, difficulty) is cd = (t / 2) % (3 C).
__device__ __forceinline__ int task_of(int metric, int n_classes, int local) { return metric * n_classes * 6 + local; }

// compute_statistics_jit(compute_fp=False) of every task of one (frame, metric): each GT not flagged -1, in order, takes
// the highest-scoring unassigned detection (first index on ties) with overlap > min_overlap; a pair with a flag of 1 on
// either side is only assigned, the others write their score into the task's segment at the frame's GT rows.
__global__ void __launch_bounds__(256) kitti_pass1_kernel(pda_kitti_frames_t fr, const double* __restrict__ ov, KittiArgs a,
                                                          const int8_t* __restrict__ gt_flags,
                                                          const int8_t* __restrict__ dt_flags, float* __restrict__ seg,
                                                          int64_t* ntp, int32_t* status) {
    __shared__ double lds[KE_LDS_DOUBLES];
    const int f = blockIdx.x, metric = blockIdx.y, lane = lane_id(), wave = threadIdx.x >> 6;
    const EvalFrame F = load_kframe(fr, f, status);
    const double* blk = stage_block(ov + (int64_t)metric * fr.ov_cap, F, lds);
    for (int local = wave; local < a.n_classes * 6; local += 4) {
        const int cd = local >> 1, k = local & 1, c = cd / 3;
        const int task = task_of(metric, a.n_classes, local);
        const double thr = a.min_overlap[k][metric][c];
        const int8_t* gfl = gt_flags + (int64_t)cd * fr.n_gt_total;
        uint64_t acc, ign;
        det_masks(dt_flags + (int64_t)cd * fr.det_cap, F, acc, ign);
        const int n_tp = match_first_pass<ScoreFloorKitti>(blk, F.ng, F.nd, fr.dt_score + F.d0, acc, ign, thr,
                                                           [&](int i) { return (int)gfl[F.g0 + i]; },
                                                           seg + (int64_t)task * fr.n_gt_total + F.g0);
        if (lane == 0 && n_tp) atomicAdd((unsigned long long*)&ntp[task], (unsigned long long)n_tp);
    }
}

// get_thresholds of one task over its n TP scores, sorted descending: score i is taken unless
// (r_recall - current_recall) < (current_recall - l_recall) and i is not the last, current_recall advanced by repeated
// += 1 / 40.0 per take, all float64.  A wave tests 64 ranks at once against the current level.
__global__ void __launch_bounds__(64) kitti_thresh_kernel(const float* __restrict__ sorted, int64_t n_gt_total,
                                                          const int64_t* ntp, const int64_t* num_valid_gt, int n_classes,
                                                          double* thresholds, int64_t* n_thr, int32_t* status) {
    const int task = blockIdx.x, lane = lane_id();
    const int64_t n = ntp[task];
    const double g = (double)num_valid_gt[(task >> 1) % (n_classes * 3)];
    const float* sc = sorted + (int64_t)task * n_gt_total;
    double* out = thresholds + (int64_t)task * KE_NS;
    const double inc = 1.0 / (KE_NS - 1.0);
    double level = 0.0;
    int64_t nt = 0;
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t i = base + lane;
        const double l = (double)(i + 1) / g;
        const double r = i < n - 1 ? (double)(i + 2) / g : l;
        int64_t cursor = base;
        while (true) {
            const bool skip = ((r - level) < (level - l)) && i < n - 1;
            const uint64_t take = __ballot(i < n && i >= cursor && !skip);
            if (!take) break;
            const int p = (int)__builtin_ctzll(take);
            if (lane == 0 && nt < KE_NS) out[nt] = (double)sc[base + p];
            ++nt;
            level += inc;
            cursor = base + p + 1;
        }
    }
    if (lane == 0) {
        n_thr[task] = nt > KE_NS ? KE_NS : nt;
        if (nt > KE_NS) atomicOr(status, 4);
    }
}

// compute_statistics_jit(compute_fp=True) of every (task, threshold) of one (frame, metric).  Per GT: the detection of
// the largest overlap among ignored_det == 0, else the first ignored_det == 1 (the assigned_ignored_det walk); then the
// fp count, DontCare suppression (metric 0) and, for metric 0 with compute_aos, the similarity sum in GT order.
__global__ void __launch_bounds__(256) kitti_pass2_kernel(pda_kitti_frames_t fr, const double* __restrict__ ov, KittiArgs a,
                                                          const int8_t* __restrict__ gt_flags,
                                                          const int8_t* __restrict__ dt_flags,
                                                          const double* __restrict__ dc_max,
                                                          const double* __restrict__ thresholds,
                                                          const int64_t* __restrict__ n_thr, int64_t* counts,
                                                          double* __restrict__ sim_frames, int32_t* status) {
    __shared__ double lds[KE_LDS_DOUBLES];
    const int f = blockIdx.x, metric = blockIdx.y, lane = lane_id(), wave = threadIdx.x >> 6;
    const EvalFrame F = load_kframe(fr, f, status);
    const double* blk = stage_block(ov + (int64_t)metric * fr.ov_cap, F, lds);
    const bool aos = metric == 0 && a.compute_aos;
    const int n_items = a.n_classes * 6 * KE_NS;
    for (int item = wave; item < n_items; item += 4) {
        const int local = item / KE_NS, t = item % KE_NS;
        const int task = task_of(metric, a.n_classes, local);
        const int nt = (int)n_thr[task];
        if (t >= nt) continue;
        const int cd = local >> 1, k = local & 1, c = cd / 3;
        const double thr = a.min_overlap[k][metric][c];
        const double th = thresholds[(int64_t)task * KE_NS + t];
        const int8_t* gfl = gt_flags + (int64_t)cd * fr.n_gt_total;
        uint64_t acc, ign;
        det_masks(dt_flags + (int64_t)cd * fr.det_cap, F, acc, ign);
        double sim = 0.0;  // the AOS similarity of the frame's true positives, summed in GT order
        const MatchStats r = match_second_pass(
            blk, F.ng, F.nd, fr.dt_score + F.d0, acc, ign, thr, th, [&](int i) { return (int)gfl[F.g0 + i]; },
            [&](int i, int jd) {
                if (aos) {
                    const double delta = fr.gt_alpha[F.g0 + i] - (double)fr.dt_alpha[F.d0 + jd];
                    sim += (1.0 + cos(delta)) / 2.0;
                }
            });
        const int tp = r.tp, fn = r.fn;
        int fp = wave_sum_i32(__builtin_popcountll(r.open));
        if (metric == 0) {
            int nstuff = 0;
            for (uint64_t m = r.open; m; m &= m - 1) {
                const int q = (int)__builtin_ctzll(m);
                nstuff += dc_max[F.d0 + lane + 64 * q] > thr;
            }
            fp -= wave_sum_i32(nstuff);
        }
        if (lane == 0) {
            int64_t* cn = counts + ((int64_t)task * KE_NS + t) * 3;
            if (tp) atomicAdd((unsigned long long*)&cn[0], (unsigned long long)tp);
            if (fp) atomicAdd((unsigned long long*)&cn[1], (unsigned long long)(int64_t)fp);
            if (fn) atomicAdd((unsigned long long*)&cn[2], (unsigned long long)fn);
            if (aos) sim_frames[((int64_t)local * KE_NS + t) * fr.n_frames + f] = sim;
        }
    }
}

// pr[t, 3] += similarity, frame after frame: one thread per (metric-0 task, threshold), a fixed order.
__global__ void __launch_bounds__(64) kitti_sim_kernel(const double* __restrict__ sim_frames, int n_frames, int n_local,
                                                       const int64_t* __restrict__ n_thr, double* similarity) {
    const int it = blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= n_local * KE_NS) return;
    const int local = it / KE_NS, t = it % KE_NS;
    double s = 0.0;
    if (t < n_thr[local]) {
        const double* p = sim_frames + (int64_t)it * n_frames;
        for (int f = 0; f < n_frames; ++f) s += p[f];
    }
    similarity[it] = s;
}

// generate_prediction_dicts' geometry of one prediction, float32 like the reference's float32 calibration:
// boxes3d_lidar_to_kitti_camera (z lowered by h / 2, lidar_to_rect = [x y z 1] (V2C^T R0^T), r = -r - pi / 2), the 8
// corners of boxes3d_to_corners3d_kitti_camera through rect_to_img (divided by the rect z), their min / max clipped to
// the image, and alpha = -arctan2(-y, x) + ry.
__global__ void __launch_bounds__(256) kitti_pred_kernel(const float* __restrict__ boxes, int64_t n, int stride,
                                                         int rows_per_frame, const int32_t* __restrict__ frame_idx,
                                                         const float* __restrict__ calib,
                                                         const int32_t* __restrict__ image_shape, int n_frames,
                                                         float* __restrict__ cam, float* __restrict__ bbox,
                                                         float* __restrict__ alpha, int32_t* status) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int64_t f = frame_idx ? (int64_t)frame_idx[r] : r / rows_per_frame;
    if (f < 0 || f >= n_frames) {
        atomicOr(status, 1);
        return;
    }
    const float* b = boxes + r * stride;
    const float* P2 = calib + f * KE_CALIB;
    const float* R0 = P2 + 12;
    const float* V2C = R0 + 9;
    const float x = b[0], y = b[1], z = b[2] - b[5] / 2, l = b[3], w = b[4], h = b[5];
    // M = V2C^T R0^T (4 x 3), then [x y z 1] M
    float M[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[k][j] = (V2C[k] * R0[3 * j] + V2C[4 + k] * R0[3 * j + 1]) + V2C[8 + k] * R0[3 * j + 2];
    float c[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = ((x * M[0][j] + y * M[1][j]) + z * M[2][j]) + M[3][j];
    const float ry = -b[6] - (float)(M_PI / 2);
    float* co = cam + r * 7;
    co[0] = c[0];
    co[1] = c[1];
    co[2] = c[2];
    co[3] = l;
    co[4] = h;
    co[5] = w;
    co[6] = ry;
    const float cr = (float)cos((double)ry), sr = (float)sin((double)ry);
    const float xs[8] = {l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2};
    const float zs[8] = {w / 2, -w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2};
    float u0 = INFINITY, v0 = INFINITY, u1 = -INFINITY, v1 = -INFINITY;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float px = c[0] + (xs[q] * cr + zs[q] * sr);
        const float py = c[1] + (q < 4 ? 0.0f : -h);
        const float pz = c[2] + (-xs[q] * sr + zs[q] * cr);
        const float u = ((px * P2[0] + py * P2[1]) + pz * P2[2]) + P2[3];
        const float v = ((px * P2[4] + py * P2[5]) + pz * P2[6]) + P2[7];
        const float iu = u / pz, iv = v / pz;
        u0 = fminf(u0, iu);
        v0 = fminf(v0, iv);
        u1 = fmaxf(u1, iu);
        v1 = fmaxf(v1, iv);
    }
    const float wmax = (float)(image_shape[2 * f + 1] - 1), hmax = (float)(image_shape[2 * f] - 1);
    float* bo = bbox + r * 4;
    bo[0] = fminf(fmaxf(u0, 0.0f), wmax);
    bo[1] = fminf(fmaxf(v0, 0.0f), hmax);
    bo[2] = fminf(fmaxf(u1, 0.0f), wmax);
    bo[3] = fminf(fmaxf(v1, 0.0f), hmax);
    alpha[r] = -(float)atan2(-(double)y, (double)x) + ry;
}

// ---- host side --------------------------------------------------------------------------------------------------------
struct Workspace {
    int64_t seg, ntp, dc, sim, total;
};

Workspace layout(int n_frames, int64_t n_gt_total, int64_t det_cap, int n_classes) {
    auto al = [](int64_t b) { return (b + 255) / 256 * 256; };
    const int64_t T = (int64_t)n_classes * 18;
    Workspace w;
    w.seg = 0;
    w.ntp = w.seg + al(T * n_gt_total * 4);
    w.dc = w.ntp + al(T * 8);
    w.sim = w.dc + al(det_cap * 8);
    w.total = w.sim + al((int64_t)n_classes * 6 * KE_NS * n_frames * 8);
    return w;
}

int check_frames(const pda_kitti_frames_t* fr, const char* what) {
    PDA_REQUIRE(fr, "%s: null frames", what);
    if (int st = check_frame_limits(what, "max_det", fr->n_frames, fr->max_gt, fr->max_det, fr->n_gt_total, fr->det_cap,
                                    fr->ov_cap))
        return st;
    PDA_REQUIRE(fr->n_gt_total <= ((int64_t)1 << 31) && fr->det_cap <= ((int64_t)1 << 31), "%s: sizes outside [0, 2^31]",
                what);
    if (fr->n_frames == 0) return PDA_OK;
    PDA_REQUIRE(fr->gt_offsets && fr->dt_start && fr->dt_count && fr->ov_start, "%s: null frame arrays", what);
    PDA_REQUIRE((fr->gt_bbox && fr->gt_loc && fr->gt_dims && fr->gt_ry && fr->gt_alpha && fr->gt_trunc && fr->gt_occ &&
                 fr->gt_name) || fr->n_gt_total == 0,
                "%s: null GT arrays", what);
    PDA_REQUIRE((fr->dt_bbox && fr->dt_box && fr->dt_alpha && fr->dt_score && fr->dt_name) || fr->det_cap == 0,
                "%s: null detection arrays", what);
    return PDA_OK;
}

int make_args(KittiArgs& a, int n_classes, int n_names, const int8_t* gt_class, const uint8_t* dt_class,
              const uint8_t* dontcare, const double* min_overlaps, int compute_aos, const char* what) {
    PDA_REQUIRE(n_classes >= 1 && n_classes <= KE_MAX_CLASSES, "%s: n_classes %d outside [1, %d]", what, n_classes,
                KE_MAX_CLASSES);
    PDA_REQUIRE(n_names >= 1 && n_names <= KE_MAX_NAMES, "%s: n_names %d outside [1, %d]", what, n_names, KE_MAX_NAMES);
    PDA_REQUIRE(gt_class && dt_class && dontcare && min_overlaps, "%s: null class tables or min_overlaps", what);
    a = KittiArgs{};
    for (int c = 0; c < n_classes; ++c)
        for (int n = 0; n < n_names; ++n) {
            const int v = gt_class[c * n_names + n];
            PDA_REQUIRE(v >= -1 && v <= 1, "%s: gt_class[%d][%d] = %d outside {-1, 0, 1}", what, c, n, v);
            a.gt_class[c][n] = (int8_t)v;
            if (dt_class[c * n_names + n]) a.dt_class[c] |= 1ull << n;
        }
    for (int n = 0; n < n_names; ++n)
        if (dontcare[n]) a.dontcare |= 1ull << n;
    for (int s = 0; s < 2; ++s)
        for (int m = 0; m < 3; ++m)
            for (int c = 0; c < n_classes; ++c) {
                const double v = min_overlaps[(s * 3 + m) * n_classes + c];
                PDA_REQUIRE(v >= 0.0 && v <= 1.0, "%s: min_overlap %g outside [0, 1]", what, v);
                a.min_overlap[s][m][c] = v;
            }
    a.n_classes = n_classes;
    a.n_names = n_names;
    a.compute_aos = compute_aos ? 1 : 0;
    return PDA_OK;
}

}  // namespace
}  // namespace pda

PDA_API int64_t pda_kitti_eval_workspace_bytes(int n_frames, int64_t n_gt_total, int64_t det_cap, int n_classes) {
    if (n_frames < 0 || n_frames > (1 << 24) || n_gt_total < 0 || n_gt_total > ((int64_t)1 << 31) || det_cap < 0 ||
        det_cap > ((int64_t)1 << 31) || n_classes < 1 || n_classes > pda::KE_MAX_CLASSES)
        return -1;
    return pda::layout(n_frames, n_gt_total, det_cap, n_classes).total;
}

PDA_API int pda_kitti_eval_overlaps(const pda_kitti_frames_t* fr, double* overlaps, int32_t* status, pda_stream_t stream) {
    const char* what = "pda_kitti_eval_overlaps";
    if (int st = pda::check_frames(fr, what)) return st;
    PDA_REQUIRE(status, "%s: null status", what);
    if (fr->n_frames == 0) return PDA_OK;
    PDA_REQUIRE(overlaps || fr->ov_cap == 0, "%s: null overlaps", what);
    const int64_t pairs = (int64_t)fr->max_gt * fr->max_det;
    if (pairs == 0) return PDA_OK;
    hipLaunchKernelGGL(pda::kitti_overlap_kernel, dim3((unsigned)fr->n_frames, (unsigned)pda::divup64(pairs, 256)), dim3(256),
                       0, (hipStream_t)stream, *fr, overlaps, status);
    return pda::check_launch(what);
}

PDA_API int pda_kitti_eval_first_pass(const pda_kitti_frames_t* fr, const double* overlaps, int n_classes, int n_names,
                                      const int8_t* gt_class, const uint8_t* dt_class, const uint8_t* dontcare,
                                      const double* min_overlaps, int8_t* gt_flags, int8_t* dt_flags,
                                      int64_t* num_valid_gt, int32_t* status, void* workspace, pda_stream_t stream) {
    const char* what = "pda_kitti_eval_first_pass";
    if (int st = pda::check_frames(fr, what)) return st;
    pda::KittiArgs a;
    if (int st = pda::make_args(a, n_classes, n_names, gt_class, dt_class, dontcare, min_overlaps, 0, what)) return st;
    PDA_REQUIRE(workspace && num_valid_gt && status, "%s: null workspace, num_valid_gt or status", what);
    PDA_REQUIRE((gt_flags || fr->n_gt_total == 0) && (dt_flags || fr->det_cap == 0), "%s: null flags", what);
    PDA_REQUIRE(overlaps || fr->ov_cap == 0, "%s: null overlaps", what);
    const pda::Workspace w = pda::layout(fr->n_frames, fr->n_gt_total, fr->det_cap, n_classes);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int T = n_classes * 18;
    if (hipMemsetAsync(ws + w.ntp, 0, T * 8, st) != hipSuccess ||
        hipMemsetAsync(num_valid_gt, 0, n_classes * 3 * 8, st) != hipSuccess)
        return pda::check_launch(what);
    if (fr->n_frames == 0) return PDA_OK;
    hipLaunchKernelGGL(pda::kitti_flags_kernel, dim3((unsigned)fr->n_frames), dim3(256), 0, st, *fr, a, gt_flags, dt_flags,
                       (double*)(ws + w.dc), num_valid_gt, status);
    hipLaunchKernelGGL(pda::kitti_pass1_kernel, dim3((unsigned)fr->n_frames, 3u), dim3(256), 0, st, *fr, overlaps, a, gt_flags,
                       dt_flags, (float*)(ws + w.seg), (int64_t*)(ws + w.ntp), status);
    return pda::check_launch(what);
}

PDA_API int pda_kitti_eval_match(const pda_kitti_frames_t* fr, const double* overlaps, int n_classes, int n_names,
                                 const int8_t* gt_class, const uint8_t* dt_class, const uint8_t* dontcare,
                                 const double* min_overlaps, int compute_aos, const int8_t* gt_flags,
                                 const int8_t* dt_flags, const float* sorted_scores, const int64_t* num_valid_gt,
                                 double* thresholds, int64_t* n_thresholds, int64_t* counts, double* similarity,
                                 int32_t* status, void* workspace, pda_stream_t stream) {
    const char* what = "pda_kitti_eval_match";
    if (int st = pda::check_frames(fr, what)) return st;
    pda::KittiArgs a;
    if (int st = pda::make_args(a, n_classes, n_names, gt_class, dt_class, dontcare, min_overlaps, compute_aos, what))
        return st;
    PDA_REQUIRE(workspace && num_valid_gt && thresholds && n_thresholds && counts && similarity && status,
                "%s: null workspace or output", what);
    PDA_REQUIRE((gt_flags || fr->n_gt_total == 0) && (dt_flags || fr->det_cap == 0), "%s: null flags", what);
    PDA_REQUIRE(sorted_scores || fr->n_gt_total == 0, "%s: null sorted_scores", what);
    PDA_REQUIRE(overlaps || fr->ov_cap == 0, "%s: null overlaps", what);
    const pda::Workspace w = pda::layout(fr->n_frames, fr->n_gt_total, fr->det_cap, n_classes);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int T = n_classes * 18, n_local = n_classes * 6;
    if (hipMemsetAsync(counts, 0, (size_t)T * pda::KE_NS * 3 * 8, st) != hipSuccess) return pda::check_launch(what);
    hipLaunchKernelGGL(pda::kitti_thresh_kernel, dim3((unsigned)T), dim3(64), 0, st, sorted_scores, fr->n_gt_total,
                       (const int64_t*)(ws + w.ntp), num_valid_gt, n_classes, thresholds, n_thresholds, status);
    if (fr->n_frames > 0)
        hipLaunchKernelGGL(pda::kitti_pass2_kernel, dim3((unsigned)fr->n_frames, 3u), dim3(256), 0, st, *fr, overlaps, a,
                           gt_flags, dt_flags, (const double*)(ws + w.dc), thresholds, n_thresholds, counts,
                           (double*)(ws + w.sim), status);
    if (compute_aos && fr->n_frames > 0)
        hipLaunchKernelGGL(pda::kitti_sim_kernel, dim3((unsigned)pda::divup64((int64_t)n_local * pda::KE_NS, 64)), dim3(64),
                           0, st, (const double*)(ws + w.sim), fr->n_frames, n_local, n_thresholds, similarity);
    else if (hipMemsetAsync(similarity, 0, (size_t)n_local * pda::KE_NS * 8, st) != hipSuccess)
        return pda::check_launch(what);
    return pda::check_launch(what);
}

PDA_API int pda_kitti_eval_predictions(const float* boxes, int64_t n, int stride, int rows_per_frame,
                                       const int32_t* frame_idx, const float* calib, const int32_t* image_shape,
                                       int n_frames, float* cam, float* bbox, float* alpha, int32_t* status,
                                       pda_stream_t stream) {
    const char* what = "pda_kitti_eval_predictions";
    PDA_REQUIRE(n >= 0 && n <= ((int64_t)1 << 31), "%s: n %lld outside [0, 2^31]", what, (long long)n);
    PDA_REQUIRE(stride >= 7, "%s: stride %d < 7", what, stride);
    PDA_REQUIRE(n_frames >= 0 && n_frames <= (1 << 24), "%s: n_frames %d outside [0, 2^24]", what, n_frames);
    PDA_REQUIRE(frame_idx || rows_per_frame >= 1, "%s: rows_per_frame %d < 1 without frame_idx", what, rows_per_frame);
    PDA_REQUIRE(status, "%s: null status", what);
    if (n == 0) return PDA_OK;
    PDA_REQUIRE(boxes && calib && image_shape && cam && bbox && alpha, "%s: null array", what);
    hipLaunchKernelGGL(pda::kitti_pred_kernel, dim3((unsigned)pda::divup64(n, 256)), dim3(256), 0, (hipStream_t)stream, boxes,
                       n, stride, rows_per_frame, frame_idx, calib, image_shape, n_frames, cam, bbox, alpha, status);
    return pda::check_launch(what);
}
