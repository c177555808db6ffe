// rotated_inter.h -- the rotated-rectangle intersection area of the numba.cuda evaluations (ONCE iou_utils.py, KITTI
// rotate_iou.py), shared by once_eval.hip and kitti_eval.hip.  Both restate the same algorithm (corners, point in
// quadrilateral, edge crossings, pseudo-angle vertex sort, fan area) and differ only in the point-in-quadrilateral
// test, which is the template parameter: InQuadCross (the sign of the four edge cross products, ONCE's live definition)
// or InQuadProj (the projections onto two edges, KITTI's point_in_quadrilateral).
//
// All of it is float32 in the reference's operation order except where numba promotes: a float32 meeting an int or
// float literal becomes float64.  That is exact for the halvings (x_d / 2, the centroid division rounds once either
// way, triangle / 2.0) and matters in one place: area() accumulates the triangle areas in float64 (area_val = 0.0).
// cos / sin are taken in double and rounded, i.e. correctly rounded float32 values.  Include after pda_common.h, inside
// no namespace.
#pragma once

namespace pda {

constexpr int RI_MAX_POLY = 24;  // 8 corners inside the other box + 16 edge crossings (the references keep 8)

__device__ __forceinline__ void rbox_corners(float* c, float x, float y, float xd, float yd, float ang) {
    const float ac = (float)cos((double)ang), as = (float)sin((double)ang);
    const float cx[4] = {-xd / 2, -xd / 2, xd / 2, xd / 2};
    const float cy[4] = {-yd / 2, yd / 2, yd / 2, -yd / 2};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[2 * i] = (ac * cx[i] + as * cy[i]) + x;
        c[2 * i + 1] = (-as * cx[i] + ac * cy[i]) + y;
    }
}

struct InQuadCross {
    static __device__ __forceinline__ bool test(float px, float py, const float* c) {
        const float pa0 = c[0] - px, pa1 = c[1] - py, pb0 = c[2] - px, pb1 = c[3] - py;
        const float pc0 = c[4] - px, pc1 = c[5] - py, pd0 = c[6] - px, pd1 = c[7] - py;
        const float pab = pa0 * pb1 - pb0 * pa1, pbc = pb0 * pc1 - pc0 * pb1;
        const float pcd = pc0 * pd1 - pd0 * pc1, pda = pd0 * pa1 - pa0 * pd1;
        return (pab >= 0 && pbc >= 0 && pcd >= 0 && pda >= 0) || (pab <= 0 && pbc <= 0 && pcd <= 0 && pda <= 0);
    }
};

struct InQuadProj {
    static __device__ __forceinline__ bool test(float px, float py, const float* c) {
        const float ab0 = c[2] - c[0], ab1 = c[3] - c[1], ad0 = c[6] - c[0], ad1 = c[7] - c[1];
        const float ap0 = px - c[0], ap1 = py - c[1];
        const float abab = ab0 * ab0 + ab1 * ab1, abap = ab0 * ap0 + ab1 * ap1;
        const float adad = ad0 * ad0 + ad1 * ad1, adap = ad0 * ap0 + ad1 * ap1;
        return abab >= abap && abap >= 0 && adad >= adap && adap >= 0;
    }
};

__device__ __forceinline__ bool segment_cross(const float* p1, const float* p2, int i, int j, float* out) {
    const float a0 = p1[2 * i], a1 = p1[2 * i + 1], b0 = p1[2 * ((i + 1) & 3)], b1 = p1[2 * ((i + 1) & 3) + 1];
    const float c0 = p2[2 * j], c1 = p2[2 * j + 1], d0 = p2[2 * ((j + 1) & 3)], d1 = p2[2 * ((j + 1) & 3) + 1];
    const float ba0 = b0 - a0, ba1 = b1 - a1, da0 = d0 - a0, ca0 = c0 - a0, da1 = d1 - a1, ca1 = c1 - a1;
    const bool acd = da1 * ca0 > ca1 * da0;
    const bool bcd = (d1 - b1) * (c0 - b0) > (c1 - b1) * (d0 - b0);
    if (acd == bcd) return false;
    const bool abc = ca1 * ba0 > ba1 * ca0;
    const bool abd = da1 * ba0 > ba1 * da0;
    if (abc == abd) return false;
    const float dc0 = d0 - c0, dc1 = d1 - c1;
    const float abba = a0 * b1 - b0 * a1, cddc = c0 * d1 - d0 * c1;
    const float dh = ba1 * dc0 - ba0 * dc1;
    const float dx = abba * dc0 - ba0 * cddc, dy = abba * dc1 - ba1 * cddc;
    out[0] = dx / dh;
    out[1] = dy / dh;
    return true;
}

// inter(rbox1, rbox2) of the references: the intersection area of two (x, y, x_d, y_d, angle) boxes in float64, before
// any store rounds it.
template <class InQuad>
__device__ double rotated_intersection_area(const float* q, const float* g) {
    float c1[8], c2[8], pts[2 * RI_MAX_POLY], vs[RI_MAX_POLY];
    rbox_corners(c1, q[0], q[1], q[2], q[3], q[4]);
    rbox_corners(c2, g[0], g[1], g[2], g[3], g[4]);
    int n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (InQuad::test(c1[2 * i], c1[2 * i + 1], c2)) { pts[2 * n] = c1[2 * i]; pts[2 * n + 1] = c1[2 * i + 1]; ++n; }
        if (InQuad::test(c2[2 * i], c2[2 * i + 1], c1)) { pts[2 * n] = c2[2 * i]; pts[2 * n + 1] = c2[2 * i + 1]; ++n; }
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float t[2];
            if (segment_cross(c1, c2, i, j, t)) { pts[2 * n] = t[0]; pts[2 * n + 1] = t[1]; ++n; }
        }
    if (n == 0) return 0.0;
    // sort_vertex_in_convex_polygon: pseudo-angle insertion sort around the centroid
    float cx = 0.0f, cy = 0.0f;
    for (int i = 0; i < n; ++i) { cx += pts[2 * i]; cy += pts[2 * i + 1]; }
    cx /= (float)n;
    cy /= (float)n;
    for (int i = 0; i < n; ++i) {
        float v0 = pts[2 * i] - cx, v1 = pts[2 * i + 1] - cy;
        const float d = __builtin_sqrtf(v0 * v0 + v1 * v1);
        v0 = v0 / d;
        v1 = v1 / d;
        if (v1 < 0) v0 = -2.0f - v0;
        vs[i] = v0;
    }
    for (int i = 1; i < n; ++i) {
        if (vs[i - 1] > vs[i]) {
            const float tv = vs[i], tx = pts[2 * i], ty = pts[2 * i + 1];
            int j = i;
            while (j > 0 && vs[j - 1] > tv) {
                vs[j] = vs[j - 1];
                pts[2 * j] = pts[2 * j - 2];
                pts[2 * j + 1] = pts[2 * j - 1];
                --j;
            }
            vs[j] = tv;
            pts[2 * j] = tx;
            pts[2 * j + 1] = ty;
        }
    }
    // area(): fan triangulation, |triangle| each, accumulated in float64 (numba: area_val = 0.0, x / 2.0)
    double a = 0.0;
    for (int i = 0; i + 2 < n; ++i) {
        const float* b = pts + 2 * i + 2;
        const float* c = pts + 2 * i + 4;
        const float t = (pts[0] - c[0]) * (b[1] - c[1]) - (pts[1] - c[1]) * (b[0] - c[0]);
        a += fabs((double)t / 2.0);
    }
    return a;
}

}  // namespace pda
