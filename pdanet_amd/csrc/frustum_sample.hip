// frustum_sample.hip -- CaDDN's FrustumToVoxel without the frustum tensor, and DDNLoss in one pass
// (include/pda_train.h: pda_frustum_sample_fwd / _bwd, pda_ddn_loss_fwd_bwd).
//
// The reference forms frustum = softmax(depth_logits)[:, :-1] x image_features (B, C, D, Hf, Wf), a (B, X, Y, Z, 3) grid
// through kornia, and a 5-D grid_sample.  The trilinear sample of an outer product factorises: a voxel needs 4 pixel
// corners with their bilinear weights, and per corner the 2-tap interpolation of the depth distribution along D.  Those
// four products W_k serve every channel, so the forward reads prob 8 times and feat 4 C times per voxel and writes the
// voxel tensor, nothing else.  One thread per voxel, consecutive lanes on consecutive X: the stores of a channel are whole
// lines, and neighbouring lanes look along nearly one ray, so their gathers hit the same few pixels.
//
// Backward (atomic formulation): the corners are recomputed.  grad_feat[c][corner k] += W_k g_c and, with
// s_k = sum_c feat[c][corner k] g_c kept in registers, grad_prob[d'][corner k] += w_uv(k) w_d(d') s_k.  Lanes of a 16-lane
// row that share the base cell form runs (neighbouring X = neighbouring depths of one ray); a segmented scan over the row
// (DPP row_shr, no LDS) adds a run up and its last lane issues the one atomic.
//
// The library is built with -fno-honor-nans: finiteness is decided on the bits, and the square root / logarithm of the
// depth bins never sees an argument outside its domain.
#include "pda_common.h"
#include "loss_sums.h"

namespace pda {

struct FsParams {
    float vg[16];                  // grid -> lidar: diag(voxel_size) with pc_min in the last column, row-major
    int c, d, hf, wf, gx, gy, gz, mode;
    float depth_min, bin, sid_lo, sid_den;
};

__device__ __forceinline__ bool fs_finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// transform_utils.bin_depths (target=False): the continuous bin index of a depth; false where the reference's value is
// not finite (the square root of a negative, the logarithm of a non-positive, a depth that is not finite).
__device__ __forceinline__ bool fs_bin_index(float depth, int mode, float depth_min, float bin, float sid_lo, float sid_den,
                                             int num_bins, float& index) {
    index = 0.f;
    if (!fs_finite_bits(depth)) return false;
    if (mode == 0) {
        index = (depth - depth_min) / bin;
    } else if (mode == 1) {
        const float arg = 1.0f + 8.0f * (depth - depth_min) / bin;
        if (!fs_finite_bits(arg) || arg < 0.f) return false;
        index = -0.5f + 0.5f * __builtin_sqrtf(arg);
    } else {
        const float arg = 1.0f + depth;
        if (!fs_finite_bits(arg) || arg <= 0.f) return false;
        index = (float)num_bins * (logf(arg) - sid_lo) / sid_den;
    }
    return fs_finite_bits(index);
}

// grid_sample's un-normalisation (align_corners=False) of a normalised coordinate that is finite or already -2, then the
// two corners: i0 = floor, weights (i0 + 1) - x and x - i0.  false: both corners lie outside [0, size).
__device__ __forceinline__ bool fs_axis(float norm, int size, int& i0, float& w0, float& w1) {
    if (!fs_finite_bits(norm)) norm = -2.0f;
    const float x = ((norm + 1.0f) * (float)size - 1.0f) / 2.0f;
    i0 = -2; w0 = w1 = 0.f;
    if (!fs_finite_bits(x) || !(x > -1.0f && x < (float)size)) return false;   // x == -1: the upper corner's weight is 0
    const float f = __builtin_floorf(x);
    i0 = (int)f;
    w0 = (f + 1.0f) - x;
    w1 = x - f;
    return true;
}

struct FsCorners {
    int off[4];        // v' * wf + u' of the pixel corners (nw, ne, sw, se), -1 outside the map
    float wuv[4];
    int x0, y0, z0;    // base cell; z0 in [-1, d - 1]
    float wz[2];
    bool zin[2];
    bool any;          // false: the voxel samples nothing
};

// Steps 1-9 of include/pda_train.h for voxel (i, j, k) of scene b.  The matrices are wave-uniform loads.
__device__ __forceinline__ void fs_corners(const FsParams& p, const float* __restrict__ l2c, const float* __restrict__ c2i,
                                           const float* __restrict__ image_hw, int b, int i, int j, int k, FsCorners& cr) {
    const float* cv = l2c + (size_t)b * 16;
    const float* ic = c2i + (size_t)b * 12;
    const float gxyz[4] = {(float)i + 0.5f, (float)j + 0.5f, (float)k + 0.5f, 1.0f};
    float cam[4];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        float acc = 0.f;
#pragma unroll
        for (int col = 0; col < 4; ++col) {
            // trans = lidar_to_cam @ grid_to_lidar first, every product of the sum kept (an infinity times a zero is a NaN)
            const float t = ((cv[r * 4 + 0] * p.vg[0 * 4 + col] + cv[r * 4 + 1] * p.vg[1 * 4 + col]) +
                             cv[r * 4 + 2] * p.vg[2 * 4 + col]) + cv[r * 4 + 3] * p.vg[3 * 4 + col];
            acc = col == 0 ? t * gxyz[col] : acc + t * gxyz[col];
        }
        cam[r] = acc;
    }
    cam[3] = 1.0f;
    float t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        t[r] = ((ic[r * 4 + 0] * cam[0] + ic[r * 4 + 1] * cam[1]) + ic[r * 4 + 2] * cam[2]) + ic[r * 4 + 3] * cam[3];
    // convert_points_from_homogeneous: 1 / z where |z| > 1e-8, else 1 (a z that is not finite divides)
    const bool divide = fs_finite_bits(t[2]) ? __builtin_fabsf(t[2]) > 1e-8f : true;
    const float s = divide ? 1.0f / t[2] : 1.0f;
    const float u = t[0] * s, v = t[1] * s;
    const float depth = t[2] - ic[2 * 4 + 3];
    float dbin;
    const bool dok = fs_bin_index(depth, p.mode, p.depth_min, p.bin, p.sid_lo, p.sid_den, p.d, dbin);
    const float h_img = image_hw[0], w_img = image_hw[1];
    const float nu = u / (w_img - 1.0f) * 2.0f + -1.0f;
    const float nv = v / (h_img - 1.0f) * 2.0f + -1.0f;
    const float nd = dok ? dbin / (float)(p.d - 1) * 2.0f + -1.0f : -2.0f;
    int x0, y0, z0;
    float wx[2], wy[2];
    const bool okx = fs_axis(nu, p.wf, x0, wx[0], wx[1]);
    const bool oky = fs_axis(nv, p.hf, y0, wy[0], wy[1]);
    const bool okz = fs_axis(nd, p.d, z0, cr.wz[0], cr.wz[1]);
    cr.any = okx && oky && okz;
    cr.x0 = x0; cr.y0 = y0; cr.z0 = z0;
    cr.zin[0] = cr.any && z0 >= 0;
    cr.zin[1] = cr.any && z0 + 1 < p.d;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int xx = x0 + (q & 1), yy = y0 + (q >> 1);
        const bool in = cr.any && xx >= 0 && xx < p.wf && yy >= 0 && yy < p.hf;
        cr.off[q] = in ? yy * p.wf + xx : -1;
        cr.wuv[q] = in ? wx[q & 1] * wy[q >> 1] : 0.f;
    }
}

// W_k = w_uv(k) * (w_d(0) prob[z0] + w_d(1) prob[z0 + 1]) at pixel corner k; prob_b: the scene's (D, Hf, Wf) block
__device__ __forceinline__ void fs_weights(const FsParams& p, const FsCorners& cr, const float* __restrict__ prob_b, float (&w)[4]) {
    const size_t plane = (size_t)p.hf * p.wf;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float a = 0.f;
        if (cr.off[q] >= 0) {
            const float p0 = cr.zin[0] ? prob_b[(size_t)cr.z0 * plane + cr.off[q]] : 0.f;
            const float p1 = cr.zin[1] ? prob_b[(size_t)(cr.z0 + 1) * plane + cr.off[q]] : 0.f;
            a = cr.wuv[q] * (cr.wz[0] * p0 + cr.wz[1] * p1);
        }
        w[q] = a;
    }
}

__global__ __launch_bounds__(256) void frustum_sample_fwd_kernel(FsParams p, const float* __restrict__ feat,
                                                                 const float* __restrict__ prob, const float* __restrict__ l2c,
                                                                 const float* __restrict__ c2i, const float* __restrict__ image_hw,
                                                                 float* __restrict__ out) {
    const int b = blockIdx.y;
    const int64_t nvox = (int64_t)p.gx * p.gy * p.gz;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;             // (k * gy + j) * gx + i
    if (n >= nvox) return;
    const int i = (int)(n % p.gx), j = (int)((n / p.gx) % p.gy), k = (int)(n / ((int64_t)p.gx * p.gy));
    FsCorners cr;
    fs_corners(p, l2c, c2i, image_hw, b, i, j, k, cr);
    const size_t plane = (size_t)p.hf * p.wf;
    float w[4];
    fs_weights(p, cr, prob + (size_t)b * p.d * plane, w);
    const float* fb = feat + (size_t)b * p.c * plane;
    float* ob = out + (size_t)b * p.c * nvox + n;
    if (!cr.any) {
        for (int ch = 0; ch < p.c; ++ch) ob[(size_t)ch * nvox] = 0.f;
        return;
    }
#pragma unroll 4
    for (int ch = 0; ch < p.c; ++ch) {
        const float* f = fb + (size_t)ch * plane;
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float v = cr.off[q] >= 0 ? f[cr.off[q]] : 0.f;
            acc += w[q] * v;
        }
        ob[(size_t)ch * nvox] = acc;
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------------
template <int CTRL> __device__ __forceinline__ float fs_row_shr(float v) {           // lane - n of the 16-lane row, else 0
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// The runs of equal keys inside each 16-lane row: which of the scan's four steps a lane takes, and whether it ends a run.
struct FsRuns {
    bool take[4], tail;
};
__device__ __forceinline__ FsRuns fs_runs(int key) {
    const int lane = lane_id();
    const int prev = __builtin_amdgcn_update_dpp(-2, key, 0x111, 0xf, 0xf, false);   // row_shr:1; -2 (no key) at a row's start
    const uint64_t heads = __ballot(prev != key);
    const int start = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));        // bit 0 is always set
    FsRuns r;
#pragma unroll
    for (int s = 0; s < 4; ++s) r.take[s] = lane - (1 << s) >= start;
    r.tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    return r;
}
// inclusive sum over the lane's run up to the lane: the run's total in its last lane
__device__ __forceinline__ float fs_run_sum(float v, const FsRuns& r) {
    float t;
    t = fs_row_shr<0x111>(v); v += r.take[0] ? t : 0.f;
    t = fs_row_shr<0x112>(v); v += r.take[1] ? t : 0.f;
    t = fs_row_shr<0x114>(v); v += r.take[2] ? t : 0.f;
    t = fs_row_shr<0x118>(v); v += r.take[3] ? t : 0.f;
    return v;
}

__global__ __launch_bounds__(256) void frustum_sample_bwd_kernel(FsParams p, const float* __restrict__ grad_out,
                                                                 const float* __restrict__ feat, const float* __restrict__ prob,
                                                                 const float* __restrict__ l2c, const float* __restrict__ c2i,
                                                                 const float* __restrict__ image_hw, float* __restrict__ grad_feat,
                                                                 float* __restrict__ grad_prob) {
    const int b = blockIdx.y;
    const int64_t nvox = (int64_t)p.gx * p.gy * p.gz;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    // every lane stays to the end: the row scans read their neighbours
    const bool live = n < nvox;
    const int64_t nn = live ? n : 0;
    const int i = (int)(nn % p.gx), j = (int)((nn / p.gx) % p.gy), k = (int)(nn / ((int64_t)p.gx * p.gy));
    FsCorners cr;
    fs_corners(p, l2c, c2i, image_hw, b, i, j, k, cr);
    if (!live) {
        cr.any = false; cr.zin[0] = cr.zin[1] = false;
#pragma unroll
        for (int q = 0; q < 4; ++q) { cr.off[q] = -1; cr.wuv[q] = 0.f; }
    }
    if (__ballot(cr.any) == 0ull) return;                                   // wave-uniform
    const size_t plane = (size_t)p.hf * p.wf;
    float w[4];
    fs_weights(p, cr, prob + (size_t)b * p.d * plane, w);
    // x0 in [-1, wf - 1], y0 in [-1, hf - 1]: (hf + 1)(wf + 1) base cells, checked against INT_MAX by the entry
    const int cell = cr.any ? (cr.y0 + 1) * (p.wf + 1) + (cr.x0 + 1) : -1;
    const FsRuns runs = fs_runs(cell);
    const float* fb = feat + (size_t)b * p.c * plane;
    float* gfb = grad_feat + (size_t)b * p.c * plane;
    const float* gob = grad_out + (size_t)b * p.c * nvox + nn;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < p.c; ++ch) {
        const float g = cr.any ? gob[(size_t)ch * nvox] : 0.f;
        const float* f = fb + (size_t)ch * plane;
        float* gf = gfb + (size_t)ch * plane;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float total = fs_run_sum(w[q] * g, runs);
            if (cr.off[q] >= 0) {
                s[q] += f[cr.off[q]] * g;
                if (runs.tail) atomicAdd(gf + cr.off[q], total);
            }
        }
    }
    // grad_prob: the runs also share the depth cell
    const int zkey = cr.any ? cr.z0 + 1 : 0;                                 // in [0, d]
    const FsRuns zruns = fs_runs(cr.any ? zkey * ((p.hf + 1) * (p.wf + 1)) + cell : -1);
    float* gpb = grad_prob + (size_t)b * p.d * plane;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int dz = 0; dz < 2; ++dz) {
            const bool in = cr.off[q] >= 0 && cr.zin[dz];
            const float total = fs_run_sum(in ? cr.wuv[q] * cr.wz[dz] * s[q] : 0.f, zruns);
            if (in && zruns.tail) atomicAdd(gpb + (size_t)(cr.z0 + dz) * plane + cr.off[q], total);
        }
    }
}

// ---- DDNLoss ----------------------------------------------------------------------------------------------------------------
struct DdnParams {
    int b, num_bins, h, w, n_boxes, mode;
    float depth_min, bin, sid_lo, sid_den, downsample;
    float alpha, gamma, fg_weight, bg_weight;
    double weight;
};
constexpr int DDN_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(256) void ddn_loss_kernel(DdnParams p, const float* __restrict__ logits,
                                                       const float* __restrict__ depth_maps, const float* __restrict__ boxes,
                                                       float* __restrict__ grad, double* __restrict__ partials) {
    const int64_t plane = (int64_t)p.h * p.w, pixels = plane * p.b;
    const int classes = p.num_bins + 1;
    const float scale = (float)(p.weight / (double)pixels);
    double sums[2] = {0.0, 0.0};                                            // foreground, background
    for (int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x; pix < pixels; pix += (int64_t)gridDim.x * 256) {
        const int b = (int)(pix / plane);
        const int64_t r = pix % plane;
        const float v = (float)(r / p.w), u = (float)(r % p.w);
        // target bin: outside [0, num_bins] or not finite -> num_bins, else truncated
        float index;
        int target = p.num_bins;
        if (fs_bin_index(depth_maps[pix], p.mode, p.depth_min, p.bin, p.sid_lo, p.sid_den, p.num_bins, index) &&
            index >= 0.f && index <= (float)p.num_bins)
            target = (int)index;
        bool fg = false;
        for (int q = 0; q < p.n_boxes; ++q) {
            const float* bx = boxes + ((size_t)b * p.n_boxes + q) * 4;
            const float u1 = __builtin_floorf(bx[0] / p.downsample), v1 = __builtin_floorf(bx[1] / p.downsample);
            const float u2 = __builtin_ceilf(bx[2] / p.downsample), v2 = __builtin_ceilf(bx[3] / p.downsample);
            fg = fg || (fs_finite_bits(u1) && fs_finite_bits(v1) && fs_finite_bits(u2) && fs_finite_bits(v2) &&
                        u >= u1 && u < u2 && v >= v1 && v < v2);
        }
        const float wpix = fg ? p.fg_weight : p.bg_weight;
        const float* x = logits + (size_t)b * classes * plane + r;
        float* gx = grad + (size_t)b * classes * plane + r;
        float m = x[0];
        for (int cls = 1; cls < classes; ++cls) m = fmaxf(m, x[(size_t)cls * plane]);
        float denom = 0.f;
        for (int cls = 0; cls < classes; ++cls) denom += expf(x[(size_t)cls * plane] - m);
        const float xt = x[(size_t)target * plane] - m;
        const float logp = xt - logf(denom);
        const float pt = expf(xt) / denom;
        const float q1 = fmaxf(1.0f - pt, 0.f);
        const float mod = powf(q1, p.gamma);                       // (1 - p_t)^gamma
        const float loss = -p.alpha * mod * logp * wpix;
        sums[fg ? 0 : 1] += (double)loss;
        // d loss / d log p_t = -alpha ((1 - p)^g - g (1 - p)^(g - 1) p log p);  d log p_t / d x_j = [j == t] - p_j
        const float dmod = q1 > 0.f ? p.gamma * powf(q1, p.gamma - 1.0f) : 0.f;
        const float coef = -p.alpha * (mod - dmod * pt * logp) * wpix * scale;
        for (int cls = 0; cls < classes; ++cls) {
            const float pj = expf(x[(size_t)cls * plane] - m) / denom;
            gx[(size_t)cls * plane] = coef * ((cls == target ? 1.0f : 0.f) - pj);
        }
    }
    block_sums_to_partials<2, 256>(sums, partials);
}

__global__ __launch_bounds__(64) void ddn_loss_finish_kernel(const double* __restrict__ partials, int blocks, double pixels,
                                                             double weight, float* __restrict__ out3) {
    double v[2];
    finish_partials<2>(partials, blocks, v);
    if (threadIdx.x == 0) {
        const double fg = v[0] / pixels, bg = v[1] / pixels;
        out3[0] = (float)((fg + bg) * weight);
        out3[1] = (float)fg;
        out3[2] = (float)bg;
    }
}

static int fs_check(const char* what, int b, int c, int d, int hf, int wf, int gx, int gy, int gz, const float* pc_min,
                    const float* voxel_size, int mode, float depth_min, float depth_max) {
    PDA_REQUIRE(b >= 0 && b <= 65535, "%s: bad size batch=%d (0..65535)", what, b);
    PDA_REQUIRE(c >= 1 && d >= 2, "%s: bad size channels=%d (>= 1) bins=%d (>= 2: the normalisation divides by bins - 1)", what, c, d);
    PDA_REQUIRE(hf >= 1 && wf >= 1 && ((int64_t)hf + 1) * ((int64_t)wf + 1) * ((int64_t)d + 1) <= 0x7fffffff,
                "%s: bad size feature map %d x %d with %d bins (at least 1 x 1, (hf + 1)(wf + 1)(bins + 1) < 2^31)", what, hf, wf, d);
    PDA_REQUIRE(gx >= 1 && gy >= 1 && gz >= 1 && (int64_t)gx * gy * gz <= (int64_t)0x7fffffff * 256,
                "%s: bad size grid %d x %d x %d", what, gx, gy, gz);
    PDA_REQUIRE(mode >= 0 && mode <= 2, "%s: bad mode %d (0 UD, 1 LID, 2 SID)", what, mode);
    PDA_REQUIRE(depth_max > depth_min, "%s: bad depth range [%g, %g]", what, (double)depth_min, (double)depth_max);
    PDA_REQUIRE(pc_min && voxel_size, "%s: null pointer (pc_min, voxel_size)", what);
    return PDA_OK;
}

// the scalars torch forms in double and applies in float32
static void fs_bins(int mode, int num_bins, double depth_min, double depth_max, float& bin, float& sid_lo, float& sid_den) {
    bin = mode == 0 ? (float)((depth_max - depth_min) / num_bins)
                    : (float)(2.0 * (depth_max - depth_min) / ((double)num_bins * (1.0 + num_bins)));
    sid_lo = (float)log(1.0 + depth_min);
    sid_den = (float)(log(1.0 + depth_max) - log(1.0 + depth_min));
}

static FsParams fs_params(int c, int d, int hf, int wf, int gx, int gy, int gz, const float* pc_min, const float* voxel_size,
                          int mode, float depth_min, float depth_max) {
    FsParams p;
    for (int q = 0; q < 16; ++q) p.vg[q] = 0.f;
    for (int q = 0; q < 3; ++q) { p.vg[q * 4 + q] = voxel_size[q]; p.vg[q * 4 + 3] = pc_min[q]; }
    p.vg[15] = 1.0f;
    p.c = c; p.d = d; p.hf = hf; p.wf = wf; p.gx = gx; p.gy = gy; p.gz = gz; p.mode = mode;
    p.depth_min = depth_min;
    fs_bins(mode, d, depth_min, depth_max, p.bin, p.sid_lo, p.sid_den);
    return p;
}

}  // namespace pda

PDA_API int pda_frustum_sample_fwd(const float* feat, const float* prob, const float* lidar_to_cam, const float* cam_to_img,
                                   const float* image_hw, float* out, int b, int c, int d, int hf, int wf, int gx, int gy, int gz,
                                   const float* pc_min, const float* voxel_size, int mode, float depth_min, float depth_max,
                                   pda_stream_t stream) {
    const int st = pda::fs_check("pda_frustum_sample_fwd", b, c, d, hf, wf, gx, gy, gz, pc_min, voxel_size, mode, depth_min, depth_max);
    if (st != PDA_OK) return st;
    if (b == 0) return PDA_OK;
    PDA_REQUIRE(feat && prob && lidar_to_cam && cam_to_img && image_hw && out, "pda_frustum_sample_fwd: null pointer");
    const pda::FsParams p = pda::fs_params(c, d, hf, wf, gx, gy, gz, pc_min, voxel_size, mode, depth_min, depth_max);
    const int64_t nvox = (int64_t)gx * gy * gz;
    hipLaunchKernelGGL(pda::frustum_sample_fwd_kernel, dim3((unsigned)pda::divup64(nvox, 256), (unsigned)b), dim3(256), 0,
                       (hipStream_t)stream, p, feat, prob, lidar_to_cam, cam_to_img, image_hw, out);
    return pda::check_launch("pda_frustum_sample_fwd");
}

PDA_API int pda_frustum_sample_bwd(const float* grad_out, const float* feat, const float* prob, const float* lidar_to_cam,
                                   const float* cam_to_img, const float* image_hw, float* grad_feat, float* grad_prob, int b,
                                   int c, int d, int hf, int wf, int gx, int gy, int gz, const float* pc_min,
                                   const float* voxel_size, int mode, float depth_min, float depth_max, pda_stream_t stream) {
    const int st = pda::fs_check("pda_frustum_sample_bwd", b, c, d, hf, wf, gx, gy, gz, pc_min, voxel_size, mode, depth_min, depth_max);
    if (st != PDA_OK) return st;
    if (b == 0) return PDA_OK;
    PDA_REQUIRE(grad_out && feat && prob && lidar_to_cam && cam_to_img && image_hw && grad_feat && grad_prob,
                "pda_frustum_sample_bwd: null pointer");
    const pda::FsParams p = pda::fs_params(c, d, hf, wf, gx, gy, gz, pc_min, voxel_size, mode, depth_min, depth_max);
    const int64_t nvox = (int64_t)gx * gy * gz;
    hipLaunchKernelGGL(pda::frustum_sample_bwd_kernel, dim3((unsigned)pda::divup64(nvox, 256), (unsigned)b), dim3(256), 0,
                       (hipStream_t)stream, p, grad_out, feat, prob, lidar_to_cam, cam_to_img, image_hw, grad_feat, grad_prob);
    return pda::check_launch("pda_frustum_sample_bwd");
}

PDA_API int64_t pda_ddn_loss_blocks(int64_t pixels) { return pda::partial_blocks(pixels, 256, pda::DDN_MAX_BLOCKS); }

PDA_API int pda_ddn_loss_fwd_bwd(const float* logits, const float* depth_maps, const float* boxes2d, float* grad_logits,
                                 double* partials, float* out3, int b, int num_bins, int h, int w, int n_boxes, int mode,
                                 float depth_min, float depth_max, float downsample, double alpha, double gamma, double fg_weight,
                                 double bg_weight, double weight, pda_stream_t stream) {
    PDA_REQUIRE(b >= 1 && h >= 1 && w >= 1 && (int64_t)b * h * w <= 0x7fffffff, "pda_ddn_loss_fwd_bwd: bad size batch=%d map %d x %d",
                b, h, w);
    PDA_REQUIRE(num_bins >= 1 && n_boxes >= 0, "pda_ddn_loss_fwd_bwd: bad size bins=%d (>= 1) boxes=%d (>= 0)", num_bins, n_boxes);
    PDA_REQUIRE(mode >= 0 && mode <= 2, "pda_ddn_loss_fwd_bwd: bad mode %d (0 UD, 1 LID, 2 SID)", mode);
    PDA_REQUIRE(depth_max > depth_min && downsample > 0.f, "pda_ddn_loss_fwd_bwd: bad depth range [%g, %g] or downsample %g",
                (double)depth_min, (double)depth_max, (double)downsample);
    PDA_REQUIRE(logits && depth_maps && grad_logits && partials && out3 && (boxes2d || n_boxes == 0),
                "pda_ddn_loss_fwd_bwd: null pointer");
    pda::DdnParams p;
    p.b = b; p.num_bins = num_bins; p.h = h; p.w = w; p.n_boxes = n_boxes; p.mode = mode;
    p.depth_min = depth_min; p.downsample = downsample;
    pda::fs_bins(mode, num_bins, depth_min, depth_max, p.bin, p.sid_lo, p.sid_den);
    p.alpha = (float)alpha; p.gamma = (float)gamma; p.fg_weight = (float)fg_weight; p.bg_weight = (float)bg_weight;
    p.weight = weight;
    const int64_t pixels = (int64_t)b * h * w;
    const int blocks = (int)pda_ddn_loss_blocks(pixels);
    hipLaunchKernelGGL(pda::ddn_loss_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, logits, depth_maps,
                       boxes2d, grad_logits, partials);
    hipLaunchKernelGGL(pda::ddn_loss_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partials, blocks, (double)pixels,
                       weight, out3);
    return pda::check_launch("pda_ddn_loss_fwd_bwd");
}
