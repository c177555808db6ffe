// box_rec.h -- the point-in-box test of roiaware_pool3d (check_pt_in_box3d), with the box's trigonometry done once into
// a record.  Shared by points_in_boxes.hip (the GPU statement: margin 1e-5, FMA under PDA_FP_CONTRACT) and augment.hip
// (the CPU statement points_in_boxes_cpu that gt_sampling's remove_points_in_boxes3d uses: margin 1e-2, no FMA).
// cos(-rz) / sin(-rz) are taken in double and rounded to float; the half-extent limits dx / 2.0 + MARGIN are the
// reference's double expressions.  fabsf(z - cz) > dz / 2.0 compares against hz = dz * 0.5f, which is exact.
#pragma once

namespace pda {

struct BoxRec {
    float cx, cy, cz, cosa, sina, hz;  // hz = dz/2 (exact in float)
    double lim_x, lim_y;               // dx/2.0 + MARGIN, dy/2.0 + MARGIN as the reference's double expression
};

// margin: the reference's float MARGIN converted to double ((double)1e-5f on the GPU, (double)1e-2f on the CPU)
__device__ __forceinline__ BoxRec make_box_rec(float cx, float cy, float cz, float dx, float dy, float dz, float rz,
                                               double margin) {
    BoxRec r;
    r.cx = cx; r.cy = cy; r.cz = cz;
    r.hz = dz * 0.5f;
    const double a = (double)(-rz);
    r.cosa = (float)cos(a);
    r.sina = (float)sin(a);
    r.lim_x = (double)dx / 2.0 + margin;
    r.lim_y = (double)dy / 2.0 + margin;
    return r;
}

template <bool FMA>
__device__ __forceinline__ bool in_box_rec(const BoxRec& r, float x, float y, float z) {
    if (fabsf(z - r.cz) > r.hz) return false;
    const float sx = x - r.cx, sy = y - r.cy;
    float lx, ly;
    if (FMA) {
        lx = __builtin_fmaf(sx, r.cosa, sy * (-r.sina));
        ly = __builtin_fmaf(sx, r.sina, sy * r.cosa);
    } else {
        lx = sx * r.cosa + sy * (-r.sina);
        ly = sx * r.sina + sy * r.cosa;
    }
    return (int)((double)fabsf(lx) < r.lim_x) & (int)((double)fabsf(ly) < r.lim_y);
}

// The same test, also handing out the local coordinates the RoI-aware pooling bins by (roiaware_pool3d_kernel.cu:52-66);
// lx / ly are written only when the z test passes.
template <bool FMA>
__device__ __forceinline__ bool in_box_rec_local(const BoxRec& r, float x, float y, float z, float& lx, float& ly) {
    if (fabsf(z - r.cz) > r.hz) return false;
    const float sx = x - r.cx, sy = y - r.cy;
    if (FMA) {
        lx = __builtin_fmaf(sx, r.cosa, sy * (-r.sina));
        ly = __builtin_fmaf(sx, r.sina, sy * r.cosa);
    } else {
        lx = sx * r.cosa + sy * (-r.sina);
        ly = sx * r.sina + sy * r.cosa;
    }
    return (int)((double)fabsf(lx) < r.lim_x) & (int)((double)fabsf(ly) < r.lim_y);
}

}  // namespace pda
