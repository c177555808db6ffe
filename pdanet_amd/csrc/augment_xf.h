// augment_xf.h -- the world transforms of the augmentor (random_flip_along_x / _y, global_rotation, global_scaling and
// limit_period of pcdet/datasets/augmentor/augmentor_utils.py), shared by augment.hip (the fixed flip -> rotate -> scale
// chain of pda_augment) and augment_steps.hip (the same operations as single steps of an ordered program), so that a
// world step rounds alike on both paths.  Every product and sum is a separately rounded float32 operation: the files
// that include this header are built with -ffp-contract=off.
#pragma once

namespace pda {

struct Xf {
    int fx, fy, rot;
    float c, s, a, sc;
};

// angle: the draw (float64); the reference's rotation angle is a float32 tensor.  angle 0 = rotation disabled: an exact
// identity.
__device__ __forceinline__ Xf xf_make(int fx, int fy, double angle, float scale) {
    Xf t;
    t.fx = fx;
    t.fy = fy;
    const float a = (float)angle;
    t.rot = a != 0.f;
    t.a = a;
    t.c = (float)cos((double)a);
    t.s = (float)sin((double)a);
    t.sc = scale;
    return t;
}

// rotate_points_along_z: [x, y, z] times [[c, s, 0], [-s, c, 0], [0, 0, 1]]
__device__ __forceinline__ void xf_rotate(float c, float s, float& x, float& y) {
    const float nx = x * c + y * (-s), ny = x * s + y * c;
    x = nx;
    y = ny;
}

// random_flip_along_x / _y, rotate_points_along_z, global_scaling
__device__ __forceinline__ void xf_point(const Xf& t, float& x, float& y, float& z) {
    if (t.fx) y = -y;
    if (t.fy) x = -x;
    if (t.rot) xf_rotate(t.c, t.s, x, y);
    x = x * t.sc;
    y = y * t.sc;
    z = z * t.sc;
}

// limit_period(h, 0.5, 2 pi) as torch's separate float32 ops
__device__ __forceinline__ float limit_heading(float h) {
    const float two_pi = 6.28318530717958647692f;
    const float q = h / two_pi + 0.5f;
    return h - floorf(q) * two_pi;
}

// the heading through the same steps, without the final limit_period
__device__ __forceinline__ float xf_heading_raw(const Xf& t, float h) {
    const float pi = 3.14159265358979323846f;
    if (t.fx) h = -h;
    if (t.fy) h = -(h + pi);
    if (t.rot) h = h + t.a;
    return h;
}

__device__ __forceinline__ float xf_heading(const Xf& t, float h) { return limit_heading(xf_heading_raw(t, h)); }

}  // namespace pda
