// iou3d_nms.hip -- rotated BEV overlap / IoU and NMS (include/pda_train.h).
//
// Reference: iou3d_nms_kernel.cu computes an N x N/64 suppression bit mask on the GPU, copies it to the
// host (cudaMemcpy = a device synchronisation per scene and per call) and runs the greedy scan on the
// CPU (iou3d_nms.cpp:90-138).  Here the scan stays on the device: one wave per scene keeps the
// "removed" bit vector in registers (lane l owns 64-box words l, l+64, ...), walks the boxes in score
// order and ORs in the mask row of every box it keeps (one coalesced 8-byte-per-lane load); all scenes
// of a batch go through one launch pair and nothing is copied to the host.  Only the upper triangle of
// the mask is computed (the scan never reads the rest).
//
// Arithmetic: float, in the reference's order (box_overlap, iou_bev, iou_normal); cos/sin/atan2 through
// double and rounded to float, exactly as oracle/pointnet2_oracle.c does (see its comment).
#include "pda_common.h"
#include "bev_overlap.h"

namespace pda {

// (na,7) x (nb,7) -> (na,nb): 64 b-boxes staged per workgroup, one thread per pair
template <bool IOU>
__global__ __launch_bounds__(256) void boxes_bev_kernel(const float* __restrict__ boxes_a, const float* __restrict__ boxes_b,
                                                        float* __restrict__ out, int na, int nb) {
    __shared__ BevBox sb[64];
    const int b0 = blockIdx.x * 64, a0 = blockIdx.y * 4;
    if ((int)threadIdx.x < 64 && b0 + (int)threadIdx.x < nb) sb[threadIdx.x] = make_box(boxes_b + (size_t)(b0 + threadIdx.x) * 7);
    __syncthreads();
    const int ai = a0 + (int)(threadIdx.x >> 6), bi = b0 + (int)(threadIdx.x & 63);
    if (ai >= na || bi >= nb) return;
    const BevBox a = make_box(boxes_a + (size_t)ai * 7);
    const BevBox& b = sb[threadIdx.x & 63];
    out[(size_t)ai * nb + bi] = IOU ? iou_bev(a, b) : box_overlap(a, b);
}

// suppression masks, upper triangle: mask[scene][i][cb] bit j = IoU(box i, box cb*64+j) > thresh, j > i
template <bool NORMAL>
__global__ __launch_bounds__(64) void nms_mask_kernel(const float* __restrict__ boxes, unsigned long long* __restrict__ mask,
                                                      int n, int col_blocks, float thresh) {
    const int col = blockIdx.x, row = blockIdx.y, scene = blockIdx.z;
    if (col < row) return;
    boxes += (size_t)scene * n * 7;
    mask += (size_t)scene * n * col_blocks;
    __shared__ BevBox sb[64];
    __shared__ float raw[64 * 7];
    const int col_size = min(n - col * 64, 64), row_size = min(n - row * 64, 64);
    if ((int)threadIdx.x < col_size) {
        const float* p = boxes + (size_t)(col * 64 + threadIdx.x) * 7;
        if (NORMAL) {
#pragma unroll
            for (int k = 0; k < 7; ++k) raw[threadIdx.x * 7 + k] = p[k];
        } else {
            sb[threadIdx.x] = make_box(p);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x >= row_size) return;
    const int i = row * 64 + threadIdx.x;
    const float* pa = boxes + (size_t)i * 7;
    BevBox a;
    if (!NORMAL) a = make_box(pa);
    unsigned long long t = 0;
    const int start = (row == col) ? (int)threadIdx.x + 1 : 0;
    for (int j = start; j < col_size; ++j) {
        const float v = NORMAL ? iou_normal(pa, raw + j * 7) : iou_bev(a, sb[j]);
        if (v > thresh) t |= 1ULL << j;
    }
    mask[(size_t)i * col_blocks + col] = t;
}

// greedy scan, one wave per scene
constexpr int SCAN_WORDS = 8;  // 64-box words per lane: n <= 64 * 64 * 8 = 32768 boxes per scene

__global__ __launch_bounds__(64) void nms_scan_kernel(const unsigned long long* __restrict__ mask, const int* __restrict__ num_valid,
                                                      long long* __restrict__ keep, int* __restrict__ num_keep, int n,
                                                      int col_blocks) {
    const int scene = blockIdx.x, lane = threadIdx.x;
    mask += (size_t)scene * n * col_blocks;
    keep += (size_t)scene * n;
    int nv = num_valid ? num_valid[scene] : n;
    nv = max(0, min(nv, n));
    unsigned long long remv[SCAN_WORDS];
#pragma unroll
    for (int w = 0; w < SCAN_WORDS; ++w) remv[w] = 0;
    int num = 0;
    for (int nb = 0; nb * 64 < nv; ++nb) {
        const int owner = nb & 63, slot = nb >> 6;
        const int in_block = min(64, nv - nb * 64);
        const unsigned long long valid = in_block == 64 ? ~0ULL : ((1ULL << in_block) - 1);
        unsigned long long mine = 0;
#pragma unroll
        for (int w = 0; w < SCAN_WORDS; ++w) if (w == slot) mine = remv[w];
        unsigned long long word = __shfl(mine, owner);
        unsigned long long avail = ~word & valid;
        while (avail) {
            const int bit = __ffsll((long long)avail) - 1;
            const int i = nb * 64 + bit;
            if (lane == 0) keep[num] = i;
            ++num;
            const unsigned long long* row = mask + (size_t)i * col_blocks;
            unsigned long long self = 0;
#pragma unroll
            for (int w = 0; w < SCAN_WORDS; ++w) {
                const int cb = w * 64 + lane;
                if (cb >= nb && cb < col_blocks) {
                    remv[w] |= row[cb];
                    if (w == slot) self = remv[w];
                }
            }
            word = __shfl(self, owner);
            const unsigned long long above = bit == 63 ? 0ULL : (~0ULL << (bit + 1));
            avail = ~word & valid & above;
        }
    }
    for (int k = num + lane; k < n; k += 64) keep[k] = -1;
    if (lane == 0) num_keep[scene] = num;
}

// multi_classes_nms' result for one scene per workgroup: the scene's c problems (head after head, class column after class
// column) each contribute their first min(num_keep, cap) kept boxes, in score order; the rows behind them are zero.
constexpr int MN_THREADS = 256;
constexpr int MN_MAX_PROBLEMS = 256;

// W: the columns of a box row, 7 + extra; pda_nms_bev itself saw a 7-column copy of the same rows.
template <int W>
__global__ __launch_bounds__(MN_THREADS) void multi_nms_compact_kernel(
        const float* __restrict__ boxes, const float* __restrict__ scores, const long long* __restrict__ keep,
        const int* __restrict__ num_keep, const int* __restrict__ label_map, int c, int k, int cap,
        float* __restrict__ pred_boxes, float* __restrict__ pred_scores, long long* __restrict__ pred_labels,
        int* __restrict__ num_pred) {
    __shared__ int first[MN_MAX_PROBLEMS + 1];
    const int scene = blockIdx.x;
    if (threadIdx.x == 0) {
        int at = 0;
        for (int p = 0; p < c; ++p) {
            first[p] = at;
            at += max(0, min(num_keep[scene * c + p], cap));
        }
        first[c] = at;
        num_pred[scene] = at;
    }
    __syncthreads();
    const int total = first[c], rows = c * cap;
    float* ob = pred_boxes + (size_t)scene * rows * W;
    float* os = pred_scores + (size_t)scene * rows;
    long long* ol = pred_labels + (size_t)scene * rows;
    for (int j = threadIdx.x; j < rows; j += MN_THREADS) {
        const int p = j / cap, r = j % cap;
        if (r < first[p + 1] - first[p]) {
            const size_t problem = (size_t)scene * c + p;
            const long long i = keep[problem * k + r];
            if (i >= 0 && i < k) {      // what pda_nms_bev wrote for r < num_keep
                const int o = first[p] + r;
                const float* src = boxes + (problem * k + (size_t)i) * W;
#pragma unroll
                for (int q = 0; q < W; ++q) ob[(size_t)o * W + q] = src[q];
                os[o] = scores[problem * k + (size_t)i];
                ol[o] = label_map[p];
            }
        }
        if (j >= total) {
#pragma unroll
            for (int q = 0; q < W; ++q) ob[(size_t)j * W + q] = 0.f;
            os[j] = 0.f;
            ol[j] = 0;
        }
    }
}

template <bool IOU>
static int launch_boxes_bev(const float* a, const float* b, float* out, int na, int nb, hipStream_t stream, const char* what) {
    PDA_REQUIRE(na >= 0 && nb >= 0, "%s: na=%d nb=%d", what, na, nb);
    if (na == 0 || nb == 0) return PDA_OK;
    PDA_REQUIRE(a && b && out, "%s: null pointer", what);
    PDA_REQUIRE(divup(na, 4) <= 65535, "%s: too many boxes_a (%d)", what, na);
    hipLaunchKernelGGL(boxes_bev_kernel<IOU>, dim3(divup(nb, 64), divup(na, 4)), dim3(256), 0, stream, a, b, out, na, nb);
    return check_launch(what);
}

}  // namespace pda

PDA_API int pda_boxes_overlap_bev(const float* boxes_a, const float* boxes_b, float* ans_overlap, int num_a, int num_b,
                                  pda_stream_t stream) {
    return pda::launch_boxes_bev<false>(boxes_a, boxes_b, ans_overlap, num_a, num_b, (hipStream_t)stream, "pda_boxes_overlap_bev");
}

PDA_API int pda_boxes_iou_bev(const float* boxes_a, const float* boxes_b, float* ans_iou, int num_a, int num_b,
                              pda_stream_t stream) {
    return pda::launch_boxes_bev<true>(boxes_a, boxes_b, ans_iou, num_a, num_b, (hipStream_t)stream, "pda_boxes_iou_bev");
}

PDA_API int64_t pda_nms_mask_words(int n) { return n <= 0 ? 0 : (int64_t)n * ((n + 63) / 64); }

PDA_API int pda_nms_bev(const float* boxes, const int32_t* num_valid, int64_t* keep, int32_t* num_keep, uint64_t* mask_scratch,
                        int b, int n, float thresh, int normal, pda_stream_t stream) {
    PDA_REQUIRE(b >= 0 && n >= 0, "pda_nms_bev: b=%d n=%d", b, n);
    if (b == 0) return PDA_OK;
    PDA_REQUIRE(keep && num_keep, "pda_nms_bev: null output");
    PDA_REQUIRE(n <= 64 * 64 * pda::SCAN_WORDS, "pda_nms_bev: %d boxes per scene > %d", n, 64 * 64 * pda::SCAN_WORDS);
    PDA_REQUIRE(b <= 65535, "pda_nms_bev: batch %d > 65535", b);
    const int cb = pda::divup(n, 64);
    if (n > 0) {
        PDA_REQUIRE(boxes && mask_scratch, "pda_nms_bev: null pointer");
        PDA_REQUIRE(cb <= 65535, "pda_nms_bev: too many boxes");
        if (normal)
            hipLaunchKernelGGL(pda::nms_mask_kernel<true>, dim3(cb, cb, b), dim3(64), 0, (hipStream_t)stream, boxes,
                               (unsigned long long*)mask_scratch, n, cb, thresh);
        else
            hipLaunchKernelGGL(pda::nms_mask_kernel<false>, dim3(cb, cb, b), dim3(64), 0, (hipStream_t)stream, boxes,
                               (unsigned long long*)mask_scratch, n, cb, thresh);
    }
    hipLaunchKernelGGL(pda::nms_scan_kernel, dim3(b), dim3(64), 0, (hipStream_t)stream, (const unsigned long long*)mask_scratch,
                       num_valid, (long long*)keep, num_keep, n, cb);
    return pda::check_launch("pda_nms_bev");
}

namespace pda {

static int multi_nms_compact(const char* what, int width, const float* boxes, const float* scores, const int64_t* keep,
                             const int32_t* num_keep, const int32_t* label_map, int b, int c, int k, int post_max,
                             float* pred_boxes, float* pred_scores, int64_t* pred_labels, int32_t* num_pred, pda_stream_t stream) {
    PDA_REQUIRE(width >= 7 && width <= 9, "%s: box_cols=%d outside 7..9", what, width);
    PDA_REQUIRE(b >= 0 && k >= 0 && post_max >= 0, "%s: b=%d k=%d post_max=%d", what, b, k, post_max);
    PDA_REQUIRE(c >= 1 && c <= MN_MAX_PROBLEMS, "%s: c=%d problems a scene outside 1..%d", what, c, MN_MAX_PROBLEMS);
    PDA_REQUIRE(b <= 65535 && (int64_t)b * c * k < ((int64_t)1 << 31) / (width > 8 ? 16 : 8), "%s: b=%d c=%d k=%d too large", what, b,
                c, k);
    if (b == 0) return PDA_OK;
    PDA_REQUIRE(num_keep && num_pred, "%s: null counts", what);
    const int cap = post_max < k ? post_max : k;      // the rows a problem can contribute
    PDA_REQUIRE(cap == 0 || (boxes && scores && keep && label_map && pred_boxes && pred_scores && pred_labels), "%s: null pointer",
                what);
    auto kernel = width == 7 ? multi_nms_compact_kernel<7> : (width == 8 ? multi_nms_compact_kernel<8> : multi_nms_compact_kernel<9>);
    hipLaunchKernelGGL(kernel, dim3(b), dim3(MN_THREADS), 0, (hipStream_t)stream, boxes, scores, (const long long*)keep, num_keep,
                       label_map, c, k, cap, pred_boxes, pred_scores, (long long*)pred_labels, num_pred);
    return check_launch(what);
}

}  // namespace pda

PDA_API int pda_multi_nms_compact(const float* boxes, const float* scores, const int64_t* keep, const int32_t* num_keep,
                                  const int32_t* label_map, int b, int c, int k, int post_max, float* pred_boxes,
                                  float* pred_scores, int64_t* pred_labels, int32_t* num_pred, pda_stream_t stream) {
    return pda::multi_nms_compact("pda_multi_nms_compact", 7, boxes, scores, keep, num_keep, label_map, b, c, k, post_max,
                                  pred_boxes, pred_scores, pred_labels, num_pred, stream);
}

PDA_API int pda_multi_nms_compact_wide(int box_cols, const float* boxes, const float* scores, const int64_t* keep,
                                       const int32_t* num_keep, const int32_t* label_map, int b, int c, int k, int post_max,
                                       float* pred_boxes, float* pred_scores, int64_t* pred_labels, int32_t* num_pred,
                                       pda_stream_t stream) {
    return pda::multi_nms_compact("pda_multi_nms_compact_wide", box_cols, boxes, scores, keep, num_keep, label_map, b, c, k,
                                  post_max, pred_boxes, pred_scores, pred_labels, num_pred, stream);
}
