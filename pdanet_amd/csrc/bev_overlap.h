// bev_overlap.h -- the rotated BEV overlap / IoU statement of iou3d_nms_kernel.cu (box_overlap, iou_bev, iou_normal),
// shared by iou3d_nms.hip (pda_boxes_overlap_bev / pda_boxes_iou_bev / pda_nms_bev) and augment.hip (gt_sampling's
// collision test).  Arithmetic: float, in the reference's order; cos/sin/atan2 through double and rounded to float,
// exactly as oracle/pointnet2_oracle.c does (see its comment).  Include after pda_common.h, inside no namespace.
#pragma once

namespace pda {

struct Pt { float x, y; };
__device__ __forceinline__ float f_cos(float a) { return (float)cos((double)a); }
__device__ __forceinline__ float f_sin(float a) { return (float)sin((double)a); }
__device__ __forceinline__ float cross2(Pt a, Pt b) { return a.x * b.y - a.y * b.x; }
__device__ __forceinline__ float cross3(Pt p1, Pt p2, Pt p0) { return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y); }
__device__ __forceinline__ float mn(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float mx(float a, float b) { return a > b ? a : b; }
constexpr float IOU_EPS = 1e-8f;

// a box with its trigonometry done once (the reference recomputes cos/sin for every pair and corner test)
struct BevBox {
    float x, y, dx, dy, c, s;  // c, s = cos/sin(heading); cos(-h) = c, sin(-h) = -s exactly
    Pt corner[4];
};

__device__ __forceinline__ Pt rot_center(Pt ctr, float c, float s, Pt p) {
    Pt r;
    r.x = (p.x - ctr.x) * c + (p.y - ctr.y) * (-s) + ctr.x;
    r.y = (p.x - ctr.x) * s + (p.y - ctr.y) * c + ctr.y;
    return r;
}

__device__ __forceinline__ BevBox make_box(const float* b) {
    BevBox r;
    r.x = b[0]; r.y = b[1]; r.dx = b[3]; r.dy = b[4];
    r.c = f_cos(b[6]); r.s = f_sin(b[6]);
    const float hx = b[3] / 2, hy = b[4] / 2;
    const Pt ctr = {b[0], b[1]};
    const Pt raw[4] = {{b[0] - hx, b[1] - hy}, {b[0] + hx, b[1] - hy}, {b[0] + hx, b[1] + hy}, {b[0] - hx, b[1] + hy}};
#pragma unroll
    for (int k = 0; k < 4; ++k) r.corner[k] = rot_center(ctr, r.c, r.s, raw[k]);
    return r;
}

__device__ __forceinline__ bool rect_cross(Pt p1, Pt p2, Pt q1, Pt q2) {
    return mn(p1.x, p2.x) <= mx(q1.x, q2.x) && mn(q1.x, q2.x) <= mx(p1.x, p2.x) && mn(p1.y, p2.y) <= mx(q1.y, q2.y) &&
           mn(q1.y, q2.y) <= mx(p1.y, p2.y);
}

__device__ __forceinline__ bool in_box2d(const BevBox& b, Pt p) {
    const float MARGIN = 1e-2f;
    // cos(-h) = cos(h), sin(-h) = -sin(h) hold exactly for correctly rounded values
    const float c = b.c, s = -b.s;
    const float rx = (p.x - b.x) * c + (p.y - b.y) * (-s);
    const float ry = (p.x - b.x) * s + (p.y - b.y) * c;
    return fabsf(rx) < b.dx / 2 + MARGIN && fabsf(ry) < b.dy / 2 + MARGIN;
}

__device__ __forceinline__ bool seg_intersection(Pt p1, Pt p0, Pt q1, Pt q0, Pt& ans) {
    if (!rect_cross(p0, p1, q0, q1)) return false;
    const float s1 = cross3(q0, p1, p0), s2 = cross3(p1, q1, p0), s3 = cross3(p0, q1, q0), s4 = cross3(q1, p1, q0);
    if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
    const float s5 = cross3(q1, p1, p0);
    if (fabsf(s5 - s1) > IOU_EPS) {
        ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float D = a0 * b1 - a1 * b0;
        ans.x = (b0 * c1 - b1 * c0) / D;
        ans.y = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

__device__ float box_overlap(const BevBox& a, const BevBox& b) {
    Pt cp[16];
    float ang[16];
    Pt center = {0.f, 0.f};
    int cnt = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            Pt x;
            if (seg_intersection(a.corner[(i + 1) & 3], a.corner[i], b.corner[(j + 1) & 3], b.corner[j], x)) {
                cp[cnt] = x;
                center.x = center.x + x.x; center.y = center.y + x.y;
                cnt++;
            }
        }
    for (int k = 0; k < 4; ++k) {
        if (in_box2d(a, b.corner[k])) { center.x = center.x + b.corner[k].x; center.y = center.y + b.corner[k].y; cp[cnt++] = b.corner[k]; }
        if (in_box2d(b, a.corner[k])) { center.x = center.x + a.corner[k].x; center.y = center.y + a.corner[k].y; cp[cnt++] = a.corner[k]; }
    }
    if (cnt < 3) return 0.f;  // no polygon: the reference's area loop yields 0 (cnt - 1 < 2 terms, all from cp[0])
    center.x /= cnt; center.y /= cnt;
    for (int i = 0; i < cnt; ++i) ang[i] = (float)atan2((double)(cp[i].y - center.y), (double)(cp[i].x - center.x));
    for (int j = 0; j < cnt - 1; ++j)
        for (int i = 0; i < cnt - j - 1; ++i)
            if (ang[i] > ang[i + 1]) {
                const Pt t = cp[i]; cp[i] = cp[i + 1]; cp[i + 1] = t;
                const float ta = ang[i]; ang[i] = ang[i + 1]; ang[i + 1] = ta;
            }
    float area = 0.f;
    for (int k = 0; k < cnt - 1; ++k) {
        const Pt u = {cp[k].x - cp[0].x, cp[k].y - cp[0].y}, v = {cp[k + 1].x - cp[0].x, cp[k + 1].y - cp[0].y};
        area += cross2(u, v);
    }
    return (float)((double)fabsf(area) / 2.0);
}

__device__ __forceinline__ float iou_bev(const BevBox& a, const BevBox& b) {
    const float sa = a.dx * a.dy, sb = b.dx * b.dy, so = box_overlap(a, b);
    return so / mx(sa + sb - so, IOU_EPS);
}

__device__ __forceinline__ float iou_normal(const float* a, const float* b) {
    const float left = mx(a[0] - a[3] / 2, b[0] - b[3] / 2), right = mn(a[0] + a[3] / 2, b[0] + b[3] / 2);
    const float top = mx(a[1] - a[4] / 2, b[1] - b[4] / 2), bottom = mn(a[1] + a[4] / 2, b[1] + b[4] / 2);
    const float w = mx(right - left, 0.f), h = mx(bottom - top, 0.f);
    const float inter = w * h, sa = a[3] * a[4], sb = b[3] * b[4];
    return inter / mx(sa + sb - inter, IOU_EPS);
}

}  // namespace pda
