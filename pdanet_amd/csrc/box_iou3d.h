// box_iou3d.h -- what recall.hip (eval) and roi_targets.hip (training) share: the reference's trimming of a scene's padded
// GT rows and its 3-D IoU of one pair, boxes_iou3d_gpu (iou3d_nms_utils.py:48-84) in float32 and torch's order.  Include
// after pda_common.h and bev_overlap.h; the including file is built with -ffp-contract=off.
#pragma once

#include <math.h>

namespace pda {

// The reference keeps rows 0..k: k starts at t - 1 and steps down while k > 0 and row k's float32 sum == 0.  Returns
// that k (0 when t == 0), the same on every lane.  The row is summed left to right; a row whose values cancel to zero only
// under some summation orders is outside the contract (torch's reduction order is not specified).  A row that holds a NaN (an
// unknown velocity) sums to NaN, which is not 0, so the row is kept: the NaN is found in the bits of the loaded values,
// because the file is built with -fno-honor-nans, under which no comparison of the sum can be relied on.
__device__ inline int trimmed_last_row(const float* __restrict__ gt, int t, int cols, int lane) {
    for (int base = t - 64; base + 63 >= 1; base -= 64) {
        const int r = base + lane;  // < t
        bool nz = false;
        if (r >= 1) {
            const float* row = gt + (size_t)r * cols;
            float s = 0.f;
            bool nan = false;
            for (int c = 0; c < cols; ++c) {
                const float v = row[c];
                nan = nan || is_nan_bits(v);
                s += nan ? 0.f : v;
            }
            nz = nan || s != 0.f;
        }
        const uint64_t m = __ballot(nz);
        if (m) return base + 63 - __clzll((long long)m);
    }
    return 0;
}

// box_overlap(a, b) is exactly 0 for a pair whose BEV circumcircles lie apart: each vertex it collects is an edge
// intersection (inside both circles) or a corner that in_box2d accepts (inside the other box widened by 1e-2 a side, so
// inside its circle widened by less than 1.5e-2).  The margin covers that and the rounding of the corners; the 3-D IoU of
// such a pair is 0 / clamp(vol_a + vol_b, 1e-6) = +0, which the caller uses without evaluating the pair.
__device__ __forceinline__ bool bev_apart(float xa, float ya, float ra, float xb, float yb, float rb) {
    const float ddx = xa - xb, ddy = ya - yb;
    const float reach = (ra + rb) * 1.0001f + 0.1f + 1e-4f * (fabsf(xa) + fabsf(ya) + fabsf(xb) + fabsf(yb));
    return ddx * ddx + ddy * ddy > reach * reach;
}

// One side of a pair: what boxes_iou3d_gpu needs of it besides the BEV polygon (make_box, built only for pairs that are
// not apart: its cos / sin go through double).
struct IouSide {
    float x, y, z_max, z_min, vol, radius;
};

__device__ __forceinline__ IouSide make_iou_side(const float* p) {
    IouSide r;
    r.x = p[0];
    r.y = p[1];
    r.z_max = p[2] + p[5] / 2;
    r.z_min = p[2] - p[5] / 2;
    r.vol = (p[3] * p[4]) * p[5];
    r.radius = 0.5f * sqrtf(p[3] * p[3] + p[4] * p[4]);
    return r;
}

__device__ __forceinline__ bool iou3d_apart(const IouSide& a, const IouSide& b) {
    return bev_apart(a.x, a.y, a.radius, b.x, b.y, b.radius);
}

// boxes_iou3d_gpu(boxes_a = a, boxes_b = b) of one pair from ov = box_overlap(a, b) in that order (not bit-symmetric): the
// height overlap, the volumes, both clamps and the division in float32 in torch's order.
__device__ __forceinline__ float iou3d_from_overlap(const IouSide& a, const IouSide& b, float ov) {
    float h = mn(a.z_max, b.z_max) - mx(a.z_min, b.z_min);
    h = h < 0.f ? 0.f : h;                                   // clamp(min=0)
    const float o3 = ov * h;
    float den = (a.vol + b.vol) - o3;
    den = den < 1e-6f ? 1e-6f : den;                         // clamp(min=1e-6)
    return o3 / den;
}

}  // namespace pda
