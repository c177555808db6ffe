// anchor_head.hip -- the anchor head of PointPillar / SECOND / PV-RCNN on the device: AxisAlignedTargetAssigner's target
// assignment (dense_heads/target_assigner/axis_aligned_target_assigner.py), AnchorHeadTemplate's three losses and box
// decoding (dense_heads/anchor_head_template.py, utils/loss_utils.py, utils/box_coder_utils.py ResidualCoder).
//
// Reference: assign_targets loops over scenes and anchor classes on the host; every iteration builds an anchors x gts IoU
// matrix, takes two argmaxes and several nonzero() compactions and writes through boolean masks; get_loss materialises
// one-hot tensors and a dozen temporaries and reads four scalars back.
//
// Here: anchor_assign_kernel<false, ..> (column maxima through an integer atomicMax on the float's bits, reduced inside the
// wave first) and anchor_assign_kernel<true, ..> (the same IoUs recomputed by the same code, labels, targets, weights, the
// positives counted with an integer atomic): no anchors x gts matrix is stored.  anchor_loss_kernel + anchor_loss_finish_kernel:
// one pass over the anchors for the three terms and their gradients, per-workgroup float64 partials summed in a fixed order
// (loss_sums.h).  anchor_decode_kernel is one launch.  No float atomics anywhere.
//
// AnchorHeadMulti (dense_heads/anchor_head_multi.py) lays its anchors out class after class (anchors.permute(3, 4, 0, 1, 2, 5),
// concatenated): anchor_assign_kernel<.., true> takes an anchor's class from the row segment that holds it, and
// anchor_multi_loss_kernel runs the same per-anchor terms (anchor_loss_row) over heads whose logits have different column
// counts, the per-head tensors described by value.
#include "loss_sums.h"

#include <math.h>

namespace pda {
namespace {

constexpr int AH_THREADS = 256;
constexpr int AH_TILE = 64;           // gt rows staged in LDS at a time
constexpr int AH_MAX_SLOTS = 64;      // anchors per location, all classes
constexpr int AH_MAX_CLASSES = 32;    // anchor classes; also num_class of the loss and the heads of a multihead
constexpr int AH_MAX_BINS = 8;        // NUM_DIR_BINS
constexpr int AH_MAX_CODE = 10;       // columns of a box code: 6 + cos, sin + two custom columns

struct AnchorAssignCfg {
    int b, m, cols, n_anchors, slots, n_cls;
    int label[AH_MAX_CLASSES];          // the 1-based gt label of each anchor class
    float matched[AH_MAX_CLASSES];
    float unmatched[AH_MAX_CLASSES];
    // location-major: class c owns the slots [first[c], first[c + 1]) of every location; class-major (SEGMENTED): the rows
    // [first[c], first[c + 1]) of the table
    int first[AH_MAX_CLASSES + 1];
};

// box_utils.boxes3d_lidar_to_aligned_bev_boxes, every operation a separate float32 one (the file is built with
// -ffp-contract=off): r = |ry - floor(ry / pi + 0.5) * pi|, dims swapped when !(r < pi / 4), corners c -+ dim / 2.
__device__ __forceinline__ void aligned_bev(float x, float y, float dx, float dy, float ry, float& x1, float& y1, float& x2,
                                            float& y2) {
    const float pi = (float)M_PI;
    const float r = fabsf(ry - floorf(ry / pi + 0.5f) * pi);
    const bool keep = r < (float)(M_PI / 4);
    const float cx = keep ? dx : dy, cy = keep ? dy : dx;
    const float hx = cx / 2.f, hy = cy / 2.f;
    x1 = x - hx;
    y1 = y - hy;
    x2 = x + hx;
    y2 = y + hy;
}

// box_utils.boxes_iou_normal for one pair
__device__ __forceinline__ float iou_normal(float ax1, float ay1, float ax2, float ay2, float area_a, float bx1, float by1,
                                            float bx2, float by2, float area_b) {
    const float x_min = fmaxf(ax1, bx1), x_max = fminf(ax2, bx2);
    const float y_min = fmaxf(ay1, by1), y_max = fminf(ay2, by2);
    const float x_len = fmaxf(x_max - x_min, 0.f), y_len = fmaxf(y_max - y_min, 0.f);
    const float inter = x_len * y_len;
    return inter / fmaxf(area_a + area_b - inter, 1e-6f);
}

// The accumulators of the two passes below, zeroed: num_pos (n_pos) and col_max (n_col, or nullptr).
__global__ __launch_bounds__(AH_THREADS) void anchor_clear_kernel(int32_t* __restrict__ num_pos, int64_t n_pos,
                                                                  uint32_t* __restrict__ col_max, int64_t n_col) {
    const int64_t i = (int64_t)blockIdx.x * AH_THREADS + threadIdx.x;
    if (i < n_pos) num_pos[i] = 0;
    if (col_max != nullptr && i < n_col) col_max[i] = 0u;
}

// SECOND == false: col_max[s, j] = max over the anchors of j's class of iou(a, j), through the bit pattern (values >= 0).
// SECOND == true: the same IoUs again; labels, targets, weights and the scene's positives.
// grid (ceil(n_anchors / 256), b); anchor n of a scene is row n of `anchors`, its class the owner of slot n % slots, or with
// SEGMENTED the owner of row n; `slot` then is the class itself.
// CODE, SINCOS (SECOND only): the width of a target row, 6 + (SINCOS ? 2 : 1) + extra, and encode_angle_by_sincos; the gt rows
// then hold 7 + extra + 1 columns, the label last.  <.., 7, false> is ResidualCoder's plain code.
template <bool SECOND, bool SEGMENTED, int CODE = 7, bool SINCOS = false>
__global__ __launch_bounds__(AH_THREADS) void anchor_assign_kernel(const float* __restrict__ anchors,
                                                                   const float* __restrict__ gt, AnchorAssignCfg g,
                                                                   uint32_t* __restrict__ col_max,
                                                                   int32_t* __restrict__ labels, float* __restrict__ targets,
                                                                   float* __restrict__ weights, int32_t* __restrict__ num_pos) {
    __shared__ float t_x1[AH_TILE], t_y1[AH_TILE], t_x2[AH_TILE], t_y2[AH_TILE], t_area[AH_TILE];
    __shared__ int t_label[AH_TILE];
    __shared__ uint32_t t_col[AH_TILE];
    __shared__ int slot_label[AH_MAX_SLOTS];
    __shared__ float slot_matched[AH_MAX_SLOTS], slot_unmatched[AH_MAX_SLOTS];
    __shared__ int seg_first[AH_MAX_CLASSES + 1];
    const int s = blockIdx.y;
    const int n = blockIdx.x * AH_THREADS + (int)threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    const bool live = n < g.n_anchors;
    if ((int)threadIdx.x < (SEGMENTED ? g.n_cls : g.slots)) {
        int c = (int)threadIdx.x;
        if (!SEGMENTED) {
            c = 0;
            while (c + 1 < g.n_cls && (int)threadIdx.x >= g.first[c + 1]) ++c;
        }
        slot_label[threadIdx.x] = g.label[c];
        slot_matched[threadIdx.x] = g.matched[c];
        slot_unmatched[threadIdx.x] = g.unmatched[c];
    }
    if (SEGMENTED && (int)threadIdx.x <= g.n_cls) seg_first[threadIdx.x] = g.first[threadIdx.x];
    float a[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
#pragma unroll
        for (int c = 0; c < 7; ++c) a[c] = anchors[(size_t)n * 7 + c];
    }
    float ax1, ay1, ax2, ay2;
    aligned_bev(a[0], a[1], a[3], a[4], a[6], ax1, ay1, ax2, ay2);
    const float area_a = (ax2 - ax1) * (ay2 - ay1);
    __syncthreads();
    int slot = 0;
    if (SEGMENTED) {
        if (live)
            while (slot + 1 < g.n_cls && n >= seg_first[slot + 1]) ++slot;
    } else if (live) {
        slot = n % g.slots;
    }
    const int my_label = live ? slot_label[slot] : -1;      // a dead lane takes part in nothing
    const float* sgt = gt + (size_t)s * g.m * g.cols;

    float row_max = -1.f;
    int row_arg = -1;
    bool forced = false;
    for (int t0 = 0; t0 < g.m; t0 += AH_TILE) {
        const int rows = min(AH_TILE, g.m - t0);
        if ((int)threadIdx.x < rows) {
            const float* row = sgt + (size_t)(t0 + threadIdx.x) * g.cols;
            float x1, y1, x2, y2;
            aligned_bev(row[0], row[1], row[3], row[4], row[6], x1, y1, x2, y2);
            t_x1[threadIdx.x] = x1;
            t_y1[threadIdx.x] = y1;
            t_x2[threadIdx.x] = x2;
            t_y2[threadIdx.x] = y2;
            t_area[threadIdx.x] = (x2 - x1) * (y2 - y1);
            const float lf = row[g.cols - 1];
            t_label[threadIdx.x] = (lf >= 1.f && lf <= 1048576.f) ? (int)lf : 0;      // 0: takes part in no class
            if (SECOND) t_col[threadIdx.x] = col_max[(size_t)s * g.m + t0 + threadIdx.x];
        }
        __syncthreads();
        for (int jj = 0; jj < rows; ++jj) {
            const bool part = t_label[jj] == my_label;
            float iou = 0.f;
            if (part) iou = iou_normal(ax1, ay1, ax2, ay2, area_a, t_x1[jj], t_y1[jj], t_x2[jj], t_y2[jj], t_area[jj]);
            if (!SECOND) {
                if (__ballot(iou > 0.f)) {      // wave-uniform: most pairs do not overlap
                    const float w = wave_max_f32(iou);
                    if (lane == 0) atomicMax(col_max + (size_t)s * g.m + t0 + jj, __float_as_uint(w));
                }
            } else if (part) {
                if (iou > row_max) {      // strict: the lowest index keeps a tie
                    row_max = iou;
                    row_arg = t0 + jj;
                }
                const uint32_t cm = t_col[jj];      // a column maximum of 0 counts as -1 and matches nothing
                forced = forced || (cm != 0u && __float_as_uint(iou) == cm);
            }
        }
        __syncthreads();
    }
    if (!SECOND) return;

    bool pos = false;
    int label = 0;
    if (live && row_arg >= 0) {
        if (forced) pos = true;
        else if (row_max < slot_unmatched[slot]) label = 0;
        else if (row_max >= slot_matched[slot]) pos = true;
        else label = -1;
    }
    if (live) {
        constexpr int ANGLE = SINCOS ? 2 : 1, EXTRA = CODE - 6 - ANGLE;
        float t[CODE];
#pragma unroll
        for (int c = 0; c < CODE; ++c) t[c] = 0.f;
        if (pos) {
            label = my_label;
            const float* row = sgt + (size_t)row_arg * g.cols;
            // ResidualCoder.encode_torch: sizes clamped to 1e-5, float32 sqrt and divisions, the logs in double
            const float dxa = fmaxf(a[3], 1e-5f), dya = fmaxf(a[4], 1e-5f), dza = fmaxf(a[5], 1e-5f);
            const float dxg = fmaxf(row[3], 1e-5f), dyg = fmaxf(row[4], 1e-5f), dzg = fmaxf(row[5], 1e-5f);
            const float diagonal = sqrtf(dxa * dxa + dya * dya);
            t[0] = (row[0] - a[0]) / diagonal;
            t[1] = (row[1] - a[1]) / diagonal;
            t[2] = (row[2] - a[2]) / dza;
            t[3] = (float)log((double)(dxg / dxa));
            t[4] = (float)log((double)(dyg / dya));
            t[5] = (float)log((double)(dzg / dza));
            if (SINCOS) {      // each cosine and sine in double, rounded once; the differences in float32
                t[6] = (float)cos((double)row[6]) - (float)cos((double)a[6]);
                t[7] = (float)sin((double)row[6]) - (float)sin((double)a[6]);
            } else {
                t[6] = row[6] - a[6];
            }
            // the custom columns against the zero columns the reference pads its anchors with: the gt's own bits
#pragma unroll
            for (int c = 0; c < EXTRA; ++c) t[6 + ANGLE + c] = row[7 + c];
        }
        const size_t e = (size_t)s * g.n_anchors + n;
        labels[e] = label;
        weights[e] = pos ? 1.f : 0.f;
#pragma unroll
        for (int c = 0; c < CODE; ++c) targets[e * CODE + c] = t[c];
    }
    const uint64_t mask = __ballot(pos);
    if (lane == 0 && mask) atomicAdd(num_pos + s, (int)__popcll(mask));
}

// ---- the three losses ----------------------------------------------------------------------------------------------------------
constexpr int AL_THREADS = 256;
constexpr int AL_PER_THREAD = 4;
constexpr int AL_MAX_BLOCKS = 2048;

struct AnchorLossCfg {
    int b, n_anchors, num_class, bins;
    float code_weight[AH_MAX_CODE];
    float dir_offset, two_pi, bin_width;      // float32 roundings of DIR_OFFSET, 2 pi, 2 pi / bins
    double cls_scale, loc_scale, dir_scale;   // weight / b
};

// The terms of one anchor, with w = 1 / max(num_pos[scene], 1):
//   cls: SigmoidFocalClassificationLoss(alpha 0.25, gamma 2) over the row's n_cols logits, the one-hot at column hot_col
//        (-1: none), weight w_cls (0 for an ignored anchor);
//   loc: WeightedSmoothL1Loss(beta 1/9), or with L1 WeightedL1Loss, over the row's CODE columns, after add_sin_difference
//        on column 6 when sin_diff (never with SINCOS, whose columns 6 and 7 are a cosine and a sine difference), weight
//        (label > 0) * w, a NaN target 0;
//   dir: softmax cross-entropy against the direction bin, weight (label > 0) * w; dp == nullptr: no direction classifier
//        (always with SINCOS).
// Every pointer is the anchor's own row.  The gradients hold d(rpn_loss) / d(prediction) for an incoming gradient of 1 and
// are written whole; s_cls, s_loc, s_dir gather the unscaled sums.
template <int CODE, bool SINCOS, bool L1>
__device__ __forceinline__ void anchor_loss_row(const AnchorLossCfg& g, int label, double w_cls, double w, int hot_col, int n_cols,
                                                bool sin_diff, const float* __restrict__ cls, const float* __restrict__ pr,
                                                const float* __restrict__ tg, const float* __restrict__ anchor,
                                                const float* __restrict__ dp, float* __restrict__ grad_cls,
                                                float* __restrict__ grad_box, float* __restrict__ grad_dir, double& s_cls,
                                                double& s_loc, double& s_dir) {
    const double beta = 1.0 / 9.0;
    for (int k = 0; k < n_cols; ++k) {
        float gr = 0.f;
        if (label >= 0) {
            const double x = (double)cls[k];
            const bool t = hot_col == k;
            const double p = 1.0 / (1.0 + exp(-x));
            const double alpha = t ? 0.25 : 0.75;
            const double pt = t ? 1.0 - p : p;
            const double bce = fmax(x, 0.0) - (t ? x : 0.0) + log1p(exp(-fabs(x)));
            s_cls += alpha * pt * pt * bce * w_cls;
            const double dpt = t ? -p * (1.0 - p) : p * (1.0 - p);
            const double dbce = p - (t ? 1.0 : 0.0);
            gr = (float)(alpha * (2.0 * pt * dpt * bce + pt * pt * dbce) * w_cls * g.cls_scale);
        }
        grad_cls[k] = gr;
    }
    // regression and direction: positives only
    float gb[CODE];
#pragma unroll
    for (int c = 0; c < CODE; ++c) gb[c] = 0.f;
    float gd[AH_MAX_BINS];
#pragma unroll
    for (int k = 0; k < AH_MAX_BINS; ++k) gd[k] = 0.f;
    if (label > 0) {
#pragma unroll
        for (int c = 0; c < CODE; ++c) {
            const float tf = tg[c];
            if (is_nan_bits(tf)) continue;
            double p = (double)pr[c], t = (double)tf, chain = 1.0;
            if (!SINCOS && c == 6 && sin_diff) {      // sin(a - b) = sin a cos b - cos a sin b, both halves differentiated in the prediction
                const double a0 = p, b0 = t;
                p = sin(a0) * cos(b0);
                t = cos(a0) * sin(b0);
                chain = cos(a0) * cos(b0) + sin(a0) * sin(b0);
            }
            const double diff = (p - t) * (double)g.code_weight[c];
            const double ad = fabs(diff);
            const double sign = diff > 0.0 ? 1.0 : (diff < 0.0 ? -1.0 : 0.0);
            s_loc += (L1 ? ad : (ad < beta ? 0.5 * ad * ad / beta : ad - 0.5 * beta)) * w;
            const double dl = L1 ? sign : (ad < beta ? diff / beta : sign);
            gb[c] = (float)(dl * (double)g.code_weight[c] * chain * w * g.loc_scale);
        }
        if (!SINCOS && dp) {
            // get_direction_target in float32, as the reference evaluates it
            const float rot_gt = tg[6] + anchor[6];
            const float val = rot_gt - g.dir_offset;
            const float offset_rot = val - floorf(val / g.two_pi + 0.f) * g.two_pi;
            int bin = (int)floorf(offset_rot / g.bin_width);
            bin = bin < 0 ? 0 : (bin > g.bins - 1 ? g.bins - 1 : bin);
            double mx = -INFINITY;
            for (int k = 0; k < g.bins; ++k) mx = fmax(mx, (double)dp[k]);
            double z = 0.0;
            for (int k = 0; k < g.bins; ++k) z += exp((double)dp[k] - mx);
            const double lse = mx + log(z);
            s_dir += (lse - (double)dp[bin]) * w;
#pragma unroll
            for (int k = 0; k < AH_MAX_BINS; ++k)
                if (k < g.bins) gd[k] = (float)((exp((double)dp[k] - lse) - (k == bin ? 1.0 : 0.0)) * w * g.dir_scale);
        }
    }
#pragma unroll
    for (int c = 0; c < CODE; ++c) grad_box[c] = gb[c];
    if (!SINCOS && dp) {
#pragma unroll
        for (int k = 0; k < AH_MAX_BINS; ++k)
            if (k < g.bins) grad_dir[k] = gd[k];
    }
}

// One anchor per thread and step over (b, n_anchors), every prediction one tensor; partials (3, blocks) the unscaled sums.
template <int CODE, bool SINCOS, bool L1>
__global__ __launch_bounds__(AL_THREADS) void anchor_loss_kernel(
        const float* __restrict__ cls_preds, const float* __restrict__ box_preds, const float* __restrict__ dir_preds,
        const int32_t* __restrict__ labels, const float* __restrict__ targets, const int32_t* __restrict__ num_pos,
        const float* __restrict__ anchors, AnchorLossCfg g, float* __restrict__ grad_cls, float* __restrict__ grad_box,
        float* __restrict__ grad_dir, double* __restrict__ partials) {
    double s_cls = 0.0, s_loc = 0.0, s_dir = 0.0;
    const long long total = (long long)g.b * g.n_anchors;
    const long long stride = (long long)gridDim.x * AL_THREADS;
    for (long long e = (long long)blockIdx.x * AL_THREADS + threadIdx.x; e < total; e += stride) {
        const int s = (int)(e / g.n_anchors);
        const int n = (int)(e % g.n_anchors);
        const int label = labels[e];
        const double w = 1.0 / (double)max(num_pos[s], 1);
        const int hot_col = label > 0 ? (g.num_class == 1 ? 0 : label - 1) : -1;      // class-agnostic: every positive is class 1
        anchor_loss_row<CODE, SINCOS, L1>(
                        g, label, w, w, hot_col, g.num_class, true, cls_preds + (size_t)e * g.num_class, box_preds + (size_t)e * CODE,
                        targets + (size_t)e * CODE, anchors + (size_t)n * 7,
                        dir_preds ? dir_preds + (size_t)e * g.bins : nullptr, grad_cls + (size_t)e * g.num_class,
                        grad_box + (size_t)e * CODE, dir_preds ? grad_dir + (size_t)e * g.bins : nullptr, s_cls, s_loc, s_dir);
    }
    const double sums[3] = {s_cls, s_loc, s_dir};
    block_sums_to_partials<3, AL_THREADS>(sums, partials);
}

// AnchorHeadMulti: head h owns the rows [row0[h], row0[h + 1]) of the class-major table and predicts them in tensors of its own,
// cls (b, rows_h, cols[h]), box (b, rows_h, CODE), dir (b, rows_h, bins); labels, targets and anchors stay (b, n_anchors, ..) and (n_anchors, 7).
struct AnchorMultiLossCfg {
    AnchorLossCfg t;                    // t.num_class: the detector's (1 = class-agnostic)
    int n_heads, sin_diff;
    double pos_w, neg_w;                // pos_cls_weight, neg_cls_weight
    int row0[AH_MAX_CLASSES + 1];
    int cols[AH_MAX_CLASSES];
    int col_base[AH_MAX_CLASSES];       // a positive of label l is hot at column l - 1 - col_base[h]
    const float* cls[AH_MAX_CLASSES];
    const float* box[AH_MAX_CLASSES];
    const float* dir[AH_MAX_CLASSES];
    float* grad_cls[AH_MAX_CLASSES];
    float* grad_box[AH_MAX_CLASSES];
    float* grad_dir[AH_MAX_CLASSES];
};

// The elements run head after head, (scene, row) inside a head, so that neighbouring threads read neighbouring rows of one
// head's tensors; the per-head descriptors are staged in LDS, where a per-thread head index costs nothing.
template <int CODE, bool SINCOS, bool L1>
__global__ __launch_bounds__(AL_THREADS) void anchor_multi_loss_kernel(const int32_t* __restrict__ labels,
                                                                        const float* __restrict__ targets,
                                                                        const int32_t* __restrict__ num_pos,
                                                                        const float* __restrict__ anchors, AnchorMultiLossCfg g,
                                                                        double* __restrict__ partials) {
    __shared__ int h_row0[AH_MAX_CLASSES + 1], h_cols[AH_MAX_CLASSES], h_base[AH_MAX_CLASSES];
    __shared__ const float* h_cls[AH_MAX_CLASSES];
    __shared__ const float* h_box[AH_MAX_CLASSES];
    __shared__ const float* h_dir[AH_MAX_CLASSES];
    __shared__ float* h_gcls[AH_MAX_CLASSES];
    __shared__ float* h_gbox[AH_MAX_CLASSES];
    __shared__ float* h_gdir[AH_MAX_CLASSES];
    if ((int)threadIdx.x < g.n_heads) {
        const int h = (int)threadIdx.x;
        h_cols[h] = g.cols[h];
        h_base[h] = g.col_base[h];
        h_cls[h] = g.cls[h];
        h_box[h] = g.box[h];
        h_dir[h] = g.dir[h];
        h_gcls[h] = g.grad_cls[h];
        h_gbox[h] = g.grad_box[h];
        h_gdir[h] = g.grad_dir[h];
    }
    if ((int)threadIdx.x <= g.n_heads) h_row0[threadIdx.x] = g.row0[threadIdx.x];
    __syncthreads();
    double s_cls = 0.0, s_loc = 0.0, s_dir = 0.0;
    const long long total = (long long)g.t.b * g.t.n_anchors;
    const long long stride = (long long)gridDim.x * AL_THREADS;
    for (long long e = (long long)blockIdx.x * AL_THREADS + threadIdx.x; e < total; e += stride) {
        int h = 0;      // head h holds the elements [b * row0[h], b * row0[h + 1])
        while (h + 1 < g.n_heads && e >= (long long)g.t.b * h_row0[h + 1]) ++h;
        const int rows = h_row0[h + 1] - h_row0[h];
        const long long local = e - (long long)g.t.b * h_row0[h];
        const int s = (int)(local / rows);
        const int r = (int)(local % rows);
        const int n = h_row0[h] + r;
        const size_t at = (size_t)s * g.t.n_anchors + n;      // in labels and targets
        const size_t hr = (size_t)s * rows + r;               // in the head's tensors
        const int label = labels[at];
        const double w = 1.0 / (double)max(num_pos[s], 1);
        const double w_cls = (label > 0 ? g.pos_w : g.neg_w) * w;
        const int c = h_cols[h];
        const int hot_col = label > 0 ? (g.t.num_class == 1 ? 0 : label - 1 - h_base[h]) : -1;
        const float* dir = h_dir[h];
        anchor_loss_row<CODE, SINCOS, L1>(
                        g.t, label, w_cls, w, hot_col, c, g.sin_diff != 0, h_cls[h] + hr * c, h_box[h] + hr * CODE, targets + at * CODE,
                        anchors + (size_t)n * 7, dir ? dir + hr * g.t.bins : nullptr, h_gcls[h] + hr * c,
                        h_gbox[h] + hr * CODE, dir ? h_gdir[h] + hr * g.t.bins : nullptr, s_cls, s_loc, s_dir);
    }
    const double sums[3] = {s_cls, s_loc, s_dir};
    block_sums_to_partials<3, AL_THREADS>(sums, partials);
}

// out = [rpn_loss_cls, rpn_loss_loc, rpn_loss_dir, rpn_loss]
__global__ __launch_bounds__(64) void anchor_loss_finish_kernel(const double* __restrict__ partials, int blocks, double cls_scale,
                                                                double loc_scale, double dir_scale, float* __restrict__ out) {
    double v[3];
    finish_partials<3>(partials, blocks, v);
    if (threadIdx.x == 0) {
        const float c = (float)(v[0] * cls_scale), l = (float)(v[1] * loc_scale), d = (float)(v[2] * dir_scale);
        out[0] = c;
        out[1] = l;
        out[2] = d;
        out[3] = c + (l + d);      // rpn_loss = cls_loss + (loc_loss + dir_loss)
    }
}

// ---- decoding ------------------------------------------------------------------------------------------------------------------
struct AnchorDecodeCfg {
    int b, n_anchors, bins;
    float dir_offset, dir_limit_offset, period;
};

// generate_predicted_boxes: ResidualCoder.decode_torch against the anchors, then the direction classifier's bin.  A code of
// CODE columns gives a box of 7 + extra, the custom columns the code's own (the anchors' are zero); with SINCOS the heading is
// atan2(sin + sin(ra), cos + cos(ra)): sin(ra) and cos(ra) in double and rounded once, the sums float32, the atan2 in double
// and rounded once, and there is no direction bin.
template <int CODE, bool SINCOS>
__global__ __launch_bounds__(256) void anchor_decode_kernel(const float* __restrict__ box_preds,
                                                            const float* __restrict__ dir_preds,
                                                            const float* __restrict__ anchors, AnchorDecodeCfg g,
                                                            float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)g.b * g.n_anchors) return;
    const int n = (int)(e % g.n_anchors);
    const float* a = anchors + (size_t)n * 7;
    constexpr int ANGLE = SINCOS ? 2 : 1, EXTRA = CODE - 6 - ANGLE;
    const float* t = box_preds + (size_t)e * CODE;
    float* o = out + (size_t)e * (7 + EXTRA);
    const float dxa = a[3], dya = a[4], dza = a[5];
    const float diagonal = sqrtf(dxa * dxa + dya * dya);
    o[0] = t[0] * diagonal + a[0];
    o[1] = t[1] * diagonal + a[1];
    o[2] = t[2] * dza + a[2];
    o[3] = (float)exp((double)t[3]) * dxa;
    o[4] = (float)exp((double)t[4]) * dya;
    o[5] = (float)exp((double)t[5]) * dza;
    float rg;
    if (SINCOS) {
        const float sn = t[7] + (float)sin((double)a[6]);
        const float cs = t[6] + (float)cos((double)a[6]);
        rg = (float)atan2((double)sn, (double)cs);
    } else {
        rg = t[6] + a[6];
    }
    if (!SINCOS && dir_preds) {
        const float* dp = dir_preds + (size_t)e * g.bins;
        int best = 0;
        float top = dp[0];
        for (int k = 1; k < g.bins; ++k)
            if (dp[k] > top) {      // strict: the lowest index keeps a tie
                top = dp[k];
                best = k;
            }
        const float val = rg - g.dir_offset;
        const float dir_rot = val - floorf(val / g.period + g.dir_limit_offset) * g.period;
        rg = (dir_rot + g.dir_offset) + g.period * (float)best;
    }
    o[6] = rg;
#pragma unroll
    for (int c = 0; c < EXTRA; ++c) o[7 + c] = t[6 + ANGLE + c] + 0.f;      // decode_torch's t + a against a zero anchor column
}

}  // namespace
}  // namespace pda

// ---- C entry points --------------------------------------------------------------------------------------------------------------
namespace pda {
namespace {

// The instantiations of a (code, sincos) pair: code = 6 + (sincos ? 2 : 1) + extra with extra in 0..2.  CALL(CODE, SINCOS) is
// expanded for the pair that holds; the callers have checked the range.
#define PDA_ANCHOR_CODED(code, sincos, CALL)     \
    switch ((code) * 2 + ((sincos) ? 1 : 0)) {   \
        case 14: CALL(7, false); break;          \
        case 16: CALL(8, false); break;          \
        case 18: CALL(9, false); break;          \
        case 17: CALL(8, true); break;           \
        case 19: CALL(9, true); break;           \
        case 21: CALL(10, true); break;          \
        default: break;                          \
    }

// Both layouts of the anchor table.  class_count: the slots a class owns at every location (location-major), or with
// `segmented` the contiguous rows it owns (class-major).  coded: the entry takes gt rows of 7 + extra + 1 columns and `sincos`.
int assign_targets(const char* what, bool segmented, bool coded, int sincos, const float* gt_boxes, int gt_cols, int b, int m, const float* anchors,
                   int n_anchors, int n_cls, const int32_t* class_label, const float* matched, const float* unmatched,
                   const int32_t* class_count, uint32_t* col_max, int32_t* box_cls_labels, float* box_reg_targets,
                   float* reg_weights, int32_t* num_pos, pda_stream_t stream) {
    PDA_REQUIRE(b >= 0 && m >= 0 && n_anchors >= 0, "%s: b=%d m=%d n_anchors=%d", what, b, m, n_anchors);
    if (coded) {
        PDA_REQUIRE(gt_cols >= 8 && gt_cols <= 10, "%s: gt_cols=%d, boxes must have 7 + extra + 1 columns with extra in 0..2", what,
                    gt_cols);
        PDA_REQUIRE(sincos == 0 || sincos == 1, "%s: sincos=%d is no flag", what, sincos);
    } else {
        PDA_REQUIRE(gt_cols == 8, "%s: gt_cols=%d, boxes must have 7 + 1 columns", what, gt_cols);
    }
    const int code = 6 + (sincos ? 2 : 1) + (gt_cols - 8);
    PDA_REQUIRE(n_cls >= 1 && n_cls <= AH_MAX_CLASSES, "%s: n_cls=%d outside 1..%d", what, n_cls, AH_MAX_CLASSES);
    PDA_REQUIRE(b <= 65535, "%s: batch %d > 65535", what, b);
    PDA_REQUIRE((int64_t)b * n_anchors < ((int64_t)1 << 31) / (code > 8 ? 16 : 8), "%s: b=%d n_anchors=%d too large", what, b,
                n_anchors);
    PDA_REQUIRE((int64_t)b * m < ((int64_t)1 << 28), "%s: b=%d m=%d too large", what, b, m);
    if (b == 0 || n_anchors == 0) return PDA_OK;
    PDA_REQUIRE(class_label && matched && unmatched && class_count, "%s: null class array", what);
    AnchorAssignCfg g{};
    g.b = b;
    g.m = m;
    g.cols = gt_cols;
    g.n_anchors = n_anchors;
    g.n_cls = n_cls;
    int64_t total = 0;
    for (int c = 0; c < n_cls; ++c) {
        PDA_REQUIRE(class_label[c] >= 1 && class_label[c] <= 1048576, "%s: class_label[%d]=%d", what, c, class_label[c]);
        for (int d = 0; d < c; ++d)
            PDA_REQUIRE(class_label[d] != class_label[c], "%s: anchor classes %d and %d share label %d", what, d, c,
                        class_label[c]);
        PDA_REQUIRE(class_count[c] >= 1 && (segmented || class_count[c] <= AH_MAX_SLOTS), "%s: class_count[%d]=%d", what, c,
                    class_count[c]);
        g.label[c] = class_label[c];
        g.matched[c] = matched[c];
        g.unmatched[c] = unmatched[c];
        g.first[c] = (int)total;
        total += class_count[c];
        PDA_REQUIRE(segmented || total <= AH_MAX_SLOTS, "%s: more than %d anchors per location", what, AH_MAX_SLOTS);
        PDA_REQUIRE(total <= n_anchors || !segmented, "%s: the classes own more than the n_anchors=%d rows of the table", what,
                    n_anchors);
    }
    g.first[n_cls] = (int)total;
    g.slots = segmented ? 0 : (int)total;
    if (segmented)
        PDA_REQUIRE(total == n_anchors, "%s: the classes own %d rows of a table of n_anchors=%d", what, (int)total, n_anchors);
    else
        PDA_REQUIRE(n_anchors % g.slots == 0, "%s: n_anchors=%d is no multiple of %d anchors per location", what, n_anchors,
                    g.slots);
    PDA_REQUIRE(anchors && box_cls_labels && box_reg_targets && reg_weights && num_pos, "%s: null pointer", what);
    PDA_REQUIRE(m == 0 || (gt_boxes && col_max), "%s: null gt_boxes or col_max", what);
    hipStream_t st = (hipStream_t)stream;
    // A kernel and not two memsets: the accumulators of a captured graph must be cleared by every replay, and memset nodes
    // did not do that reliably (MI355X: from the second replay on num_pos and col_max carried the replay before).
    const int64_t n_clear = (int64_t)b * (m > 1 ? m : 1);
    if (n_clear > 0)
        hipLaunchKernelGGL(anchor_clear_kernel, dim3((unsigned)divup64(n_clear, AH_THREADS)), dim3(AH_THREADS), 0, st, num_pos, (int64_t)b,
                           m > 0 ? col_max : (uint32_t*)nullptr, (int64_t)b * m);
    const dim3 grid(divup(n_anchors, AH_THREADS), b);
    auto first = segmented ? anchor_assign_kernel<false, true> : anchor_assign_kernel<false, false>;
    auto second = first;
#define PDA_SECOND(CODE, SINCOS) \
    second = segmented ? anchor_assign_kernel<true, true, CODE, SINCOS> : anchor_assign_kernel<true, false, CODE, SINCOS>
    PDA_ANCHOR_CODED(code, sincos, PDA_SECOND)
#undef PDA_SECOND
    if (m > 0)
        hipLaunchKernelGGL(first, grid, dim3(AH_THREADS), 0, st, anchors, gt_boxes, g, col_max, (int32_t*)nullptr,
                           (float*)nullptr, (float*)nullptr, (int32_t*)nullptr);
    hipLaunchKernelGGL(second, grid, dim3(AH_THREADS), 0, st, anchors, gt_boxes, g, col_max, box_cls_labels, box_reg_targets,
                       reg_weights, num_pos);
    return check_launch(what);
}

}  // namespace
}  // namespace pda

PDA_API int pda_anchor_assign_targets(const float* gt_boxes, int gt_cols, int b, int m, const float* anchors, int n_anchors,
                                      int n_cls, const int32_t* class_label, const float* matched, const float* unmatched,
                                      const int32_t* class_count, uint32_t* col_max, int32_t* box_cls_labels,
                                      float* box_reg_targets, float* reg_weights, int32_t* num_pos, pda_stream_t stream) {
    return pda::assign_targets("pda_anchor_assign_targets", false, false, 0, gt_boxes, gt_cols, b, m, anchors, n_anchors, n_cls, class_label,
                               matched, unmatched, class_count, col_max, box_cls_labels, box_reg_targets, reg_weights, num_pos,
                               stream);
}

PDA_API int pda_anchor_multi_assign_targets(const float* gt_boxes, int gt_cols, int b, int m, const float* anchors, int n_anchors,
                                            int n_cls, const int32_t* class_label, const float* matched, const float* unmatched,
                                            const int32_t* class_rows, uint32_t* col_max, int32_t* box_cls_labels,
                                            float* box_reg_targets, float* reg_weights, int32_t* num_pos, pda_stream_t stream) {
    return pda::assign_targets("pda_anchor_multi_assign_targets", true, false, 0, gt_boxes, gt_cols, b, m, anchors, n_anchors, n_cls,
                               class_label, matched, unmatched, class_rows, col_max, box_cls_labels, box_reg_targets, reg_weights,
                               num_pos, stream);
}

PDA_API int64_t pda_anchor_loss_blocks(int64_t n) {
    return pda::partial_blocks(n, (int64_t)pda::AL_THREADS * pda::AL_PER_THREAD, pda::AL_MAX_BLOCKS);
}

namespace pda {
namespace {

// The checks every coded entry makes on (code, sincos, reg_loss) and on sincos next to a direction classifier.
int check_code(const char* what, int code, int sincos, int reg_loss, bool has_dir) {
    PDA_REQUIRE(sincos == 0 || sincos == 1, "%s: sincos=%d is no flag", what, sincos);
    PDA_REQUIRE(code >= 7 + sincos && code <= 9 + sincos,
                "%s: code=%d outside %d..%d (6 + %d heading columns + extra, extra in 0..2)", what, code, 7 + sincos, 9 + sincos,
                1 + sincos);
    PDA_REQUIRE(reg_loss == PDA_REG_SMOOTH_L1 || reg_loss == PDA_REG_L1, "%s: reg_loss=%d is neither smooth L1 (%d) nor L1 (%d)",
                what, reg_loss, PDA_REG_SMOOTH_L1, PDA_REG_L1);
    PDA_REQUIRE(!(sincos && has_dir), "%s: sincos with dir_cls_preds (the sine difference and the direction bins need a scalar "
                "heading)", what);
    return PDA_OK;
}

int anchor_loss(const char* what, int code, int sincos, int reg_loss, const float* cls_preds, const float* box_preds,
                const float* dir_cls_preds, const int32_t* box_cls_labels, const float* box_reg_targets, const int32_t* num_pos,
                const float* anchors, int b, int n_anchors, int num_class, int bins, const float* code_weights, double cls_weight,
                double loc_weight, double dir_weight, double dir_offset, float* grad_cls, float* grad_box, float* grad_dir,
                double* partials, float* out, pda_stream_t stream) {
    PDA_REQUIRE(b >= 1 && n_anchors >= 1, "%s: b=%d n_anchors=%d", what, b, n_anchors);
    PDA_REQUIRE((int64_t)b * n_anchors < ((int64_t)1 << 31) / 32, "%s: b=%d n_anchors=%d too large", what, b, n_anchors);
    PDA_REQUIRE(num_class >= 1 && num_class <= AH_MAX_CLASSES, "%s: num_class=%d outside 1..%d", what, num_class, AH_MAX_CLASSES);
    PDA_REQUIRE(!dir_cls_preds || (bins >= 1 && bins <= AH_MAX_BINS), "%s: bins=%d outside 1..%d", what, bins, AH_MAX_BINS);
    PDA_REQUIRE(cls_preds && box_preds && box_cls_labels && box_reg_targets && num_pos && anchors && code_weights && grad_cls &&
                    grad_box && partials && out,
                "%s: null pointer", what);
    PDA_REQUIRE(!dir_cls_preds || grad_dir, "%s: null grad_dir", what);
    AnchorLossCfg g{};
    g.b = b;
    g.n_anchors = n_anchors;
    g.num_class = num_class;
    g.bins = dir_cls_preds ? bins : 0;
    for (int c = 0; c < code; ++c) g.code_weight[c] = code_weights[c];
    g.dir_offset = (float)dir_offset;
    g.two_pi = (float)(2.0 * M_PI);
    g.bin_width = (float)(2.0 * M_PI / (dir_cls_preds ? bins : 1));
    g.cls_scale = cls_weight / b;
    g.loc_scale = loc_weight / b;
    g.dir_scale = dir_cls_preds ? dir_weight / b : 0.0;
    const int blocks = (int)pda_anchor_loss_blocks((int64_t)b * n_anchors);
    auto kernel = anchor_loss_kernel<7, false, false>;
#define PDA_LOSS(CODE, SINCOS) \
    kernel = reg_loss == PDA_REG_L1 ? anchor_loss_kernel<CODE, SINCOS, true> : anchor_loss_kernel<CODE, SINCOS, false>
    PDA_ANCHOR_CODED(code, sincos, PDA_LOSS)
#undef PDA_LOSS
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(AL_THREADS), 0, (hipStream_t)stream, cls_preds, box_preds, dir_cls_preds,
                       box_cls_labels, box_reg_targets, num_pos, anchors, g, grad_cls, grad_box, grad_dir, partials);
    hipLaunchKernelGGL(anchor_loss_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partials, blocks, g.cls_scale,
                       g.loc_scale, g.dir_scale, out);
    return check_launch(what);
}

}  // namespace
}  // namespace pda

PDA_API int pda_anchor_loss(const float* cls_preds, const float* box_preds, const float* dir_cls_preds,
                            const int32_t* box_cls_labels, const float* box_reg_targets, const int32_t* num_pos,
                            const float* anchors, int b, int n_anchors, int num_class, int bins, const float* code_weights,
                            double cls_weight, double loc_weight, double dir_weight, double dir_offset, float* grad_cls,
                            float* grad_box, float* grad_dir, double* partials, float* out, pda_stream_t stream) {
    return pda::anchor_loss("pda_anchor_loss", 7, 0, PDA_REG_SMOOTH_L1, cls_preds, box_preds, dir_cls_preds, box_cls_labels,
                            box_reg_targets, num_pos, anchors, b, n_anchors, num_class, bins, code_weights, cls_weight, loc_weight,
                            dir_weight, dir_offset, grad_cls, grad_box, grad_dir, partials, out, stream);
}

PDA_API int pda_anchor_loss_coded(int code, int sincos, int reg_loss, const float* cls_preds, const float* box_preds,
                                  const float* dir_cls_preds, const int32_t* box_cls_labels, const float* box_reg_targets,
                                  const int32_t* num_pos, const float* anchors, int b, int n_anchors, int num_class, int bins,
                                  const float* code_weights, double cls_weight, double loc_weight, double dir_weight,
                                  double dir_offset, float* grad_cls, float* grad_box, float* grad_dir, double* partials,
                                  float* out, pda_stream_t stream) {
    if (int rc = pda::check_code("pda_anchor_loss_coded", code, sincos, reg_loss, dir_cls_preds != nullptr)) return rc;
    return pda::anchor_loss("pda_anchor_loss_coded", code, sincos, reg_loss, cls_preds, box_preds, dir_cls_preds, box_cls_labels,
                            box_reg_targets, num_pos, anchors, b, n_anchors, num_class, bins, code_weights, cls_weight, loc_weight,
                            dir_weight, dir_offset, grad_cls, grad_box, grad_dir, partials, out, stream);
}

PDA_API int pda_anchor_assign_targets_coded(const float* gt_boxes, int gt_cols, int sincos, int b, int m, const float* anchors,
                                            int n_anchors, int n_cls, const int32_t* class_label, const float* matched,
                                            const float* unmatched, const int32_t* class_count, uint32_t* col_max,
                                            int32_t* box_cls_labels, float* box_reg_targets, float* reg_weights, int32_t* num_pos,
                                            pda_stream_t stream) {
    return pda::assign_targets("pda_anchor_assign_targets_coded", false, true, sincos, gt_boxes, gt_cols, b, m, anchors, n_anchors,
                               n_cls, class_label, matched, unmatched, class_count, col_max, box_cls_labels, box_reg_targets,
                               reg_weights, num_pos, stream);
}

PDA_API int pda_anchor_multi_assign_targets_coded(const float* gt_boxes, int gt_cols, int sincos, int b, int m, const float* anchors,
                                                  int n_anchors, int n_cls, const int32_t* class_label, const float* matched,
                                                  const float* unmatched, const int32_t* class_rows, uint32_t* col_max,
                                                  int32_t* box_cls_labels, float* box_reg_targets, float* reg_weights,
                                                  int32_t* num_pos, pda_stream_t stream) {
    return pda::assign_targets("pda_anchor_multi_assign_targets_coded", true, true, sincos, gt_boxes, gt_cols, b, m, anchors,
                               n_anchors, n_cls, class_label, matched, unmatched, class_rows, col_max, box_cls_labels,
                               box_reg_targets, reg_weights, num_pos, stream);
}

PDA_API int64_t pda_anchor_multi_loss_blocks(int64_t n) {
    return pda::partial_blocks(n, (int64_t)pda::AL_THREADS * pda::AL_PER_THREAD, pda::AL_MAX_BLOCKS);
}

namespace pda {
namespace {

int anchor_multi_loss(const char* what, int code, int sincos, int reg_loss, const float* const* cls_preds, const float* const* box_preds, const float* const* dir_cls_preds,
                                  int n_heads, const int32_t* head_rows, const int32_t* head_cols, const int32_t* head_col_base,
                                  const int32_t* box_cls_labels, const float* box_reg_targets, const int32_t* num_pos,
                                  const float* anchors, int b, int n_anchors, int num_class, int bins, const float* code_weights,
                                  double cls_weight, double loc_weight, double dir_weight, double dir_offset, double pos_cls_weight,
                                  double neg_cls_weight, float* const* grad_cls, float* const* grad_box, float* const* grad_dir,
                                  double* partials, float* out, pda_stream_t stream) {
    PDA_REQUIRE(b >= 1 && n_anchors >= 1, "%s: b=%d n_anchors=%d", what, b, n_anchors);
    PDA_REQUIRE((int64_t)b * n_anchors < ((int64_t)1 << 31) / 32, "%s: b=%d n_anchors=%d too large", what, b, n_anchors);
    PDA_REQUIRE(n_heads >= 1 && n_heads <= AH_MAX_CLASSES, "%s: n_heads=%d outside 1..%d", what, n_heads,
                AH_MAX_CLASSES);
    PDA_REQUIRE(num_class >= 1 && num_class <= AH_MAX_CLASSES, "%s: num_class=%d outside 1..%d", what, num_class,
                AH_MAX_CLASSES);
    PDA_REQUIRE(!dir_cls_preds || (bins >= 1 && bins <= AH_MAX_BINS), "%s: bins=%d outside 1..%d", what, bins,
                AH_MAX_BINS);
    PDA_REQUIRE(cls_preds && box_preds && head_rows && head_cols && head_col_base && grad_cls && grad_box,
                "%s: null head array", what);
    PDA_REQUIRE(!dir_cls_preds || grad_dir, "%s: null grad_dir", what);
    AnchorMultiLossCfg g{};
    int64_t rows = 0;
    for (int h = 0; h < n_heads; ++h) {
        PDA_REQUIRE(head_rows[h] >= 1, "%s: head_rows[%d]=%d", what, h, head_rows[h]);
        PDA_REQUIRE(head_cols[h] >= 1 && head_col_base[h] >= 0 && head_cols[h] + head_col_base[h] <= num_class,
                    "%s: head %d has columns %d..%d of num_class=%d", what, h, head_col_base[h],
                    head_col_base[h] + head_cols[h], num_class);
        g.row0[h] = (int)rows;
        rows += head_rows[h];
        PDA_REQUIRE(rows <= n_anchors, "%s: the heads own more than the n_anchors=%d rows", what, n_anchors);
        g.cols[h] = head_cols[h];
        g.col_base[h] = head_col_base[h];
        PDA_REQUIRE(cls_preds[h] && box_preds[h] && grad_cls[h] && grad_box[h] && (!dir_cls_preds || (dir_cls_preds[h] && grad_dir[h])),
                    "%s: null pointer of head %d", what, h);
        g.cls[h] = cls_preds[h];
        g.box[h] = box_preds[h];
        g.dir[h] = dir_cls_preds ? dir_cls_preds[h] : nullptr;
        g.grad_cls[h] = grad_cls[h];
        g.grad_box[h] = grad_box[h];
        g.grad_dir[h] = dir_cls_preds ? grad_dir[h] : nullptr;
    }
    g.row0[n_heads] = (int)rows;
    PDA_REQUIRE(rows == n_anchors, "%s: the heads own %d rows of n_anchors=%d", what, (int)rows, n_anchors);
    PDA_REQUIRE(box_cls_labels && box_reg_targets && num_pos && anchors && code_weights && partials && out,
                "%s: null pointer", what);
    g.n_heads = n_heads;
    g.sin_diff = dir_cls_preds ? 1 : 0;      // anchor_head_multi.py adds the sin difference only behind a direction classifier
    g.pos_w = pos_cls_weight;
    g.neg_w = neg_cls_weight;
    g.t.b = b;
    g.t.n_anchors = n_anchors;
    g.t.num_class = num_class;
    g.t.bins = dir_cls_preds ? bins : 0;
    for (int c = 0; c < code; ++c) g.t.code_weight[c] = code_weights[c];
    g.t.dir_offset = (float)dir_offset;
    g.t.two_pi = (float)(2.0 * M_PI);
    g.t.bin_width = (float)(2.0 * M_PI / (dir_cls_preds ? bins : 1));
    g.t.cls_scale = cls_weight / b;
    g.t.loc_scale = loc_weight / b;
    g.t.dir_scale = dir_cls_preds ? dir_weight / b : 0.0;
    const int blocks = (int)pda_anchor_multi_loss_blocks((int64_t)b * n_anchors);
    auto kernel = anchor_multi_loss_kernel<7, false, false>;
#define PDA_LOSS(CODE, SINCOS) \
    kernel = reg_loss == PDA_REG_L1 ? anchor_multi_loss_kernel<CODE, SINCOS, true> : anchor_multi_loss_kernel<CODE, SINCOS, false>
    PDA_ANCHOR_CODED(code, sincos, PDA_LOSS)
#undef PDA_LOSS
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(AL_THREADS), 0, (hipStream_t)stream, box_cls_labels, box_reg_targets, num_pos,
                       anchors, g, partials);
    hipLaunchKernelGGL(anchor_loss_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partials, blocks, g.t.cls_scale,
                       g.t.loc_scale, g.t.dir_scale, out);
    return check_launch(what);
}

}  // namespace
}  // namespace pda

#define PDA_MULTI_LOSS_ARGS                                                                                                       \
    cls_preds, box_preds, dir_cls_preds, n_heads, head_rows, head_cols, head_col_base, box_cls_labels, box_reg_targets, num_pos,  \
            anchors, b, n_anchors, num_class, bins, code_weights, cls_weight, loc_weight, dir_weight, dir_offset, pos_cls_weight, \
            neg_cls_weight, grad_cls, grad_box, grad_dir, partials, out, stream

PDA_API int pda_anchor_multi_loss(const float* const* cls_preds, const float* const* box_preds, const float* const* dir_cls_preds,
                                  int n_heads, const int32_t* head_rows, const int32_t* head_cols, const int32_t* head_col_base,
                                  const int32_t* box_cls_labels, const float* box_reg_targets, const int32_t* num_pos,
                                  const float* anchors, int b, int n_anchors, int num_class, int bins, const float* code_weights,
                                  double cls_weight, double loc_weight, double dir_weight, double dir_offset, double pos_cls_weight,
                                  double neg_cls_weight, float* const* grad_cls, float* const* grad_box, float* const* grad_dir,
                                  double* partials, float* out, pda_stream_t stream) {
    return pda::anchor_multi_loss("pda_anchor_multi_loss", 7, 0, PDA_REG_SMOOTH_L1, PDA_MULTI_LOSS_ARGS);
}

PDA_API int pda_anchor_multi_loss_coded(int code, int sincos, int reg_loss, const float* const* cls_preds,
                                        const float* const* box_preds, const float* const* dir_cls_preds, int n_heads,
                                        const int32_t* head_rows, const int32_t* head_cols, const int32_t* head_col_base,
                                        const int32_t* box_cls_labels, const float* box_reg_targets, const int32_t* num_pos,
                                        const float* anchors, int b, int n_anchors, int num_class, int bins,
                                        const float* code_weights, double cls_weight, double loc_weight, double dir_weight,
                                        double dir_offset, double pos_cls_weight, double neg_cls_weight, float* const* grad_cls,
                                        float* const* grad_box, float* const* grad_dir, double* partials, float* out,
                                        pda_stream_t stream) {
    if (int rc = pda::check_code("pda_anchor_multi_loss_coded", code, sincos, reg_loss, dir_cls_preds != nullptr)) return rc;
    return pda::anchor_multi_loss("pda_anchor_multi_loss_coded", code, sincos, reg_loss, PDA_MULTI_LOSS_ARGS);
}
#undef PDA_MULTI_LOSS_ARGS

namespace pda {
namespace {

int anchor_decode(const char* what, int code, int sincos, const float* box_preds, const float* dir_cls_preds, const float* anchors,
                  int b, int n_anchors, int bins, double dir_offset, double dir_limit_offset, float* batch_box_preds,
                  pda_stream_t stream) {
    PDA_REQUIRE(b >= 0 && n_anchors >= 0 && (int64_t)b * n_anchors < ((int64_t)1 << 31) / (code > 8 ? 16 : 8), "%s: b=%d n_anchors=%d",
                what, b, n_anchors);
    PDA_REQUIRE(!dir_cls_preds || (bins >= 1 && bins <= AH_MAX_BINS), "%s: bins=%d outside 1..%d", what, bins, AH_MAX_BINS);
    if (b == 0 || n_anchors == 0) return PDA_OK;
    PDA_REQUIRE(box_preds && anchors && batch_box_preds, "%s: null pointer", what);
    AnchorDecodeCfg g{};
    g.b = b;
    g.n_anchors = n_anchors;
    g.bins = dir_cls_preds ? bins : 0;
    g.dir_offset = (float)dir_offset;
    g.dir_limit_offset = (float)dir_limit_offset;
    g.period = (float)(2.0 * M_PI / (dir_cls_preds ? bins : 1));
    auto kernel = anchor_decode_kernel<7, false>;
#define PDA_DECODE(CODE, SINCOS) kernel = anchor_decode_kernel<CODE, SINCOS>
    PDA_ANCHOR_CODED(code, sincos, PDA_DECODE)
#undef PDA_DECODE
    hipLaunchKernelGGL(kernel, dim3((unsigned)divup64((int64_t)b * n_anchors, 256)), dim3(256), 0, (hipStream_t)stream, box_preds,
                       dir_cls_preds, anchors, g, batch_box_preds);
    return check_launch(what);
}

}  // namespace
}  // namespace pda

PDA_API int pda_anchor_decode(const float* box_preds, const float* dir_cls_preds, const float* anchors, int b, int n_anchors,
                              int bins, double dir_offset, double dir_limit_offset, float* batch_box_preds,
                              pda_stream_t stream) {
    return pda::anchor_decode("pda_anchor_decode", 7, 0, box_preds, dir_cls_preds, anchors, b, n_anchors, bins, dir_offset,
                              dir_limit_offset, batch_box_preds, stream);
}

PDA_API int pda_anchor_decode_coded(int code, int sincos, const float* box_preds, const float* dir_cls_preds, const float* anchors,
                                    int b, int n_anchors, int bins, double dir_offset, double dir_limit_offset,
                                    float* batch_box_preds, pda_stream_t stream) {
    if (int rc = pda::check_code("pda_anchor_decode_coded", code, sincos, PDA_REG_SMOOTH_L1, dir_cls_preds != nullptr)) return rc;
    return pda::anchor_decode("pda_anchor_decode_coded", code, sincos, box_preds, dir_cls_preds, anchors, b, n_anchors, bins,
                              dir_offset, dir_limit_offset, batch_box_preds, stream);
}
