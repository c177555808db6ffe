// recall.hip -- the eval loop's 3-D recall bookkeeping on the device: Detector3DTemplate.generate_recall_record
// (detector3d_template.py:288-329) for every scene of a batch in one launch, summed into counters that stay on the device.
//
// Reference, per scene: trim trailing all-zero GT rows (never row 0), boxes_iou3d_gpu(final boxes, trimmed GT)
// (iou3d_nms_utils.py:48-84: one BEV kernel plus a dozen elementwise launches), then per threshold a max over the
// predictions, a compare, a sum and an .item() (a host synchronisation each).
//
// Here: one wave per (scene, GT row).  The wave finds the scene's trimmed row count with a top-down ballot over the rows,
// its lanes stride over the scene's predictions computing the 3-D IoU of (prediction, GT) in the reference's float order,
// a wave max gives the row's best IoU, and each workgroup adds its GT count and recalled counts to the counters with one
// integer atomic per counter -- order-free, so runs are bit-identical and one buffer can collect a whole epoch.
#include "pda_common.h"
#include "bev_overlap.h"
#include "box_iou3d.h"

namespace pda {
namespace {

constexpr int RECALL_MAX_THRESH = 16;
constexpr int RECALL_WAVES = 4;  // GT rows per workgroup

struct RecallThresh {
    float t[RECALL_MAX_THRESH];  // RECALL_THRESH_LIST rounded to float32: torch compares a float32 tensor in float32
};

__global__ __launch_bounds__(64 * RECALL_WAVES) void recall_record_kernel(
        const float* __restrict__ pred, const int32_t* __restrict__ num_pred, const float* __restrict__ gt, int cols,
        RecallThresh th, int n_thresh, unsigned long long* __restrict__ counters, float* __restrict__ max_iou, int k, int t) {
    __shared__ int part[RECALL_WAVES][1 + RECALL_MAX_THRESH];
    const int s = blockIdx.y, wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const float* sgt = gt + (size_t)s * t * cols;
    const int kept = trimmed_last_row(sgt, t, cols, lane) + 1;
    if ((int)blockIdx.x * RECALL_WAVES >= kept) return;  // the whole workgroup: every row it owns was trimmed
    const int g = (int)blockIdx.x * RECALL_WAVES + wave;
    const int n = min(max(num_pred[s], 0), k);
    const bool active = g < kept;
    float best = 0.f;
    if (active && n > 0) {
        // boxes_iou3d_gpu(boxes_a = predictions, boxes_b = GT): box_iou3d.h, uncontracted (this file is built with
        // -ffp-contract=off)
        const float* gr = sgt + (size_t)g * cols;
        const IouSide gb = make_iou_side(gr);
        const BevBox gbev = make_box(gr);
        float m = -INFINITY;
        for (int j = lane; j < n; j += 64) {
            const float* pa = pred + ((size_t)s * k + j) * 7;
            const IouSide a = make_iou_side(pa);
            const float iou = iou3d_apart(a, gb) ? 0.f : iou3d_from_overlap(a, gb, box_overlap(make_box(pa), gbev));
            m = iou > m ? iou : m;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float v = __shfl_xor(m, o);
            m = v > m ? v : m;
        }
        best = m;
    }
    if (lane == 0) {
        if (active && max_iou) max_iou[(size_t)s * t + g] = best;       // 0 without predictions
        part[wave][0] = active ? 1 : 0;
#pragma unroll
        for (int i = 0; i < RECALL_MAX_THRESH; ++i)
            if (i < n_thresh) part[wave][1 + i] = (active && n > 0 && best > th.t[i]) ? 1 : 0;
    }
    __syncthreads();
    if ((int)threadIdx.x <= n_thresh) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < RECALL_WAVES; ++w) sum += part[w][threadIdx.x];
        if (sum) atomicAdd(counters + threadIdx.x, (unsigned long long)sum);
    }
}

}  // namespace
}  // namespace pda

PDA_API int pda_recall_record(const float* pred_boxes, const int32_t* num_pred, const float* gt_boxes, int gt_cols,
                              const float* thresh, int n_thresh, int64_t* counters, float* max_iou, int b, int k, int t,
                              pda_stream_t stream) {
    PDA_REQUIRE(b >= 0 && k >= 0 && t >= 0, "pda_recall_record: b=%d k=%d t=%d", b, k, t);
    PDA_REQUIRE(gt_cols >= 7, "pda_recall_record: gt_cols=%d < 7", gt_cols);
    PDA_REQUIRE(n_thresh >= 0 && n_thresh <= pda::RECALL_MAX_THRESH, "pda_recall_record: n_thresh=%d outside 0..%d", n_thresh,
                pda::RECALL_MAX_THRESH);
    PDA_REQUIRE(b <= 65535, "pda_recall_record: batch %d > 65535", b);
    if (b == 0 || t == 0) return PDA_OK;
    PDA_REQUIRE(num_pred && gt_boxes && counters, "pda_recall_record: null pointer");
    PDA_REQUIRE(k == 0 || pred_boxes, "pda_recall_record: null pred_boxes");
    PDA_REQUIRE(n_thresh == 0 || thresh, "pda_recall_record: null thresh");
    pda::RecallThresh th{};
    for (int i = 0; i < n_thresh; ++i) th.t[i] = thresh[i];
    hipLaunchKernelGGL(pda::recall_record_kernel, dim3(pda::divup(t, pda::RECALL_WAVES), b), dim3(64 * pda::RECALL_WAVES), 0,
                       (hipStream_t)stream, pred_boxes, num_pred, gt_boxes, gt_cols, th, n_thresh,
                       (unsigned long long*)counters, max_iou, k, t);
    return pda::check_launch("pda_recall_record");
}
