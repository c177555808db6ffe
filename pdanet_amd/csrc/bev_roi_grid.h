// bev_roi_grid.h -- from a sampling position on a BEV map to the four corners bilinear interpolation reads
// (grid_sample, bilinear, zero padding).  Plain C++ that compiles for the host and the device: bev_roi_pool.hip samples
// with it, and tools/bev_roi_grid_check.cpp runs it under the host sanitizers on a table of hostile positions.
//
// The rule: a position that is not finite, or that lies outside [-1, w) x [-1, h), reads nothing.  The float -> int
// conversion happens only after that range check, so no NaN, infinity or 1e30 is ever converted or used as an index.
// Finiteness is decided by the bit pattern (the library is built with -fno-honor-nans).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PDA_HD __host__ __device__ __forceinline__
#else
#define PDA_HD inline
#endif

namespace pda {

struct BevCorners {
    int off[4];    // y * w + x of nw, ne, sw, se inside one (h, w) plane; -1: the corner is outside the map
    float wt[4];   // nw, ne, sw, se weights, from the unclamped position
};

PDA_HD bool bev_finite_bits(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, sizeof(u));
    return (u & 0x7f800000u) != 0x7f800000u;
}

// false: the sample reads nothing (every off is -1, every weight 0).  Needs 2 <= w, h <= 2^24, so that (float)w is exact.
PDA_HD bool bev_roi_corners(float ix, float iy, int w, int h, BevCorners& c) {
    for (int k = 0; k < 4; ++k) { c.off[k] = -1; c.wt[k] = 0.f; }
    if (!bev_finite_bits(ix) || !bev_finite_bits(iy)) return false;
    if (!(ix >= -1.0f && ix < (float)w && iy >= -1.0f && iy < (float)h)) return false;
    const float fx = __builtin_floorf(ix), fy = __builtin_floorf(iy);     // in [-1, w - 1] x [-1, h - 1]
    const int x0 = (int)fx, y0 = (int)fy;
    const float ex = (fx + 1.0f) - ix, wx = ix - fx, ey = (fy + 1.0f) - iy, wy = iy - fy;
    const bool in_x0 = x0 >= 0, in_x1 = x0 + 1 < w, in_y0 = y0 >= 0, in_y1 = y0 + 1 < h;
    c.wt[0] = ex * ey; c.wt[1] = wx * ey; c.wt[2] = ex * wy; c.wt[3] = wx * wy;
    if (in_x0 && in_y0) c.off[0] = y0 * w + x0;
    if (in_x1 && in_y0) c.off[1] = y0 * w + x0 + 1;
    if (in_x0 && in_y1) c.off[2] = (y0 + 1) * w + x0;
    if (in_x1 && in_y1) c.off[3] = (y0 + 1) * w + x0 + 1;
    return true;
}

// The reference's six theta expressions (second_head.py roi_grid_pool) and the sampling position of grid row i, column j,
// as torch evaluates them with align_corners=False: float32 throughout.  roi = [x, y, z, dx, dy, dz, ry].
struct BevTheta { float t[6]; };

PDA_HD BevTheta bev_roi_theta(const float* roi, float cosa, float sina, int w, int h, float min_x, float min_y, float cell_x,
                              float cell_y) {
    const float x1 = (roi[0] - roi[3] / 2 - min_x) / cell_x, x2 = (roi[0] + roi[3] / 2 - min_x) / cell_x;
    const float y1 = (roi[1] - roi[4] / 2 - min_y) / cell_y, y2 = (roi[1] + roi[4] / 2 - min_y) / cell_y;
    const float wm = (float)(w - 1), hm = (float)(h - 1);
    BevTheta th;
    th.t[0] = (x2 - x1) / wm * cosa;
    th.t[1] = (x2 - x1) / wm * (-sina);
    th.t[2] = (x1 + x2 - (float)w + 1) / wm;
    th.t[3] = (y2 - y1) / hm * sina;
    th.t[4] = (y2 - y1) / hm * cosa;
    th.t[5] = (y1 + y2 - (float)h + 1) / hm;
    return th;
}

PDA_HD void bev_roi_position(const BevTheta& th, int i, int j, int g, int w, int h, float& ix, float& iy) {
    const float u = (float)(2 * j + 1) / (float)g - 1.0f, v = (float)(2 * i + 1) / (float)g - 1.0f;
    const float gx = th.t[0] * u + th.t[1] * v + th.t[2], gy = th.t[3] * u + th.t[4] * v + th.t[5];
    ix = ((gx + 1.0f) * (float)w - 1.0f) / 2;
    iy = ((gy + 1.0f) * (float)h - 1.0f) / 2;
}

}  // namespace pda
