// stack_sa.hip -- one scale of StackSAModuleMSG (pointnet2_stack/pointnet2_modules.py:78-112 of the reference) with two
// Conv-BN-ReLU layers and a max pool, without its (M, 3 + C_in, nsample) grouped tensor and the (M, C, nsample) tensors
// behind it; and interpolate_from_bev_features of VoxelSetAbstraction (pda_bev_interpolate_*, at the end of the file).
//
// The first conv is split, W1 = [W1x (C1 x 3) | W1f (C1 x C_in)]: F = features W1f^T (N, C1) is one matmul over the SOURCE
// rows, made by the caller.  The kernels see F, xyz, new_xyz, the two count vectors, idx (M, ns) as pda_stack_ball_query
// leaves it (indices LOCAL to the scene, idx[i][0] = -1 for an empty ball, short lists repeat the first hit), W1x, W2 and
// per-channel (scale, shift) pairs.  The scene starts are prefix sums of the counts, made in LDS by every workgroup as
// stack_group_kernel does.  A slot reads NOTHING, and stands for rel = 0, F = 0, when its row is empty or its index lies
// outside [0, count of the centre's scene): ssa_slot is the one statement of that rule.
//
// One slot (i, s), float32, in this order (the file is built with -ffp-contract=off; the only fused operations are the
// explicit fmaf of the y2 chain):
//     rel   = xyz[g] - new_xyz[i]
//     y1[c] = F[g][c] + ((w0 rx + w1 ry) + w2 rz)                  0 in every slot of an empty row
//     z1[c] = max(s1_c y1[c] + t1_c, 0)
//     y2[d] = fma chain over c ascending of W2[d][c] z1[c], from 0
// per (i, d): the largest and the smallest y2 over s with the first slot that attains each; the one the sign of the second
// BatchNorm's weight selects is written (u, a); pda_stack_sa_apply makes out = max(s2 u + t2, 0) once s2, t2 are known.
//
// BatchNorm2d sees all n = M ns slots, padded repeats and empty rows included: sum y1, sum y1^2 (pda_stack_sa_moments) and
// sum y2, sum y2^2 (pda_stack_sa_fwd) are float64, per-workgroup partials finished in one fixed order (loss_sums.h).
//
// Backward, two recompute passes (pointnet2_stack_modules.py derives the per-channel constants A, B in float64):
//     dy2[i,s,d] = [s = a[i,d]] s2_d g[i,d] - A2_d - B2_d y2[i,s,d]
//   pass 1: dW2[d][c] = sum dy2[d] z1[c];  e1[c] = (sum_d dy2[d] W2[d][c]) [z1[c] > 0], written to HBM (M, ns, C1) -- the one
//           slot-sized tensor of the path -- with per-channel sum e1 and sum e1 y1
//   pass 2: dy1 = s1 e1 - A1 - B1 y1 for the slots that read a row:  dF[g] += dy1 (float atomicAdd, as the stacked grouping
//           backward; the only result that is not bit-reproducible), dW1x[c] = sum dy1[c] rel
// Every sum but dF is float64 partials in a fixed order; dW2 is first added in float32 inside a lane (the slots of one centre
// until the grid reaches SSA_MAX_BLOCKS workgroups, of m / (SSA_MAX_BLOCKS 256 / C2) centres beyond), then in float64.
//
// Layout.  fwd / pass 1: a workgroup takes 256 / C2 centres at a time.  Per slot, the threads first make z1 of those centres
// into LDS as (centre, c) items, then thread (centre, d) runs its chain against W2's row d held in registers; pass 1 then
// hands dy2 through LDS back to the (centre, c) items, which read W2's column c from an LDS copy.  moments / pass 2: C1
// lanes per centre, lane = channel.
#include "loss_sums.h"

namespace pda {

constexpr int SSA_THREADS = 256;
constexpr int SSA_MAX_BLOCKS = 1024;
constexpr int SSA_MAX_B = 1024;

struct SsaScenes {
    int cpre[SSA_MAX_B + 1];     // prefix sums of the centre counts
    int ppre[SSA_MAX_B + 1];     // prefix sums of the point counts
};

// called by every thread; the caller synchronises afterwards
__device__ __forceinline__ void ssa_prefix(const int* __restrict__ new_cnt, const int* __restrict__ cnt, int b, SsaScenes& sc) {
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int k = 0; k < b; ++k) { sc.cpre[k] = acc; acc += new_cnt[k]; }
        sc.cpre[b] = acc;
    }
    if (threadIdx.x == 64) {
        int acc = 0;
        for (int k = 0; k < b; ++k) { sc.ppre[k] = acc; acc += cnt[k]; }
        sc.ppre[b] = acc;
    }
}

struct SsaCentre {
    float qx, qy, qz;
    int start, count;            // the centre's scene in xyz / F, clipped to [0, n]
    const int* row;              // idx + pt * ns; nullptr: the centre reads nothing (past m, or an empty ball)
};

__device__ __forceinline__ SsaCentre ssa_centre(int64_t pt, int m, int ns, int n, int b, const int* __restrict__ idx,
                                                const float* __restrict__ new_xyz, const SsaScenes& sc) {
    SsaCentre ce;
    ce.qx = ce.qy = ce.qz = 0.f;
    ce.start = ce.count = 0;
    ce.row = nullptr;
    if (pt >= m) return ce;
    const int* row = idx + (size_t)pt * ns;
    if (row[0] < 0) return ce;
    int scene = 0;               // the scan of stack_scene (stack_ops.hip): centres past the total stay in the last scene
    for (int k = 1; k < b; ++k) scene = ((int)pt >= sc.cpre[k]) ? k : scene;
    const int lo = min(max(sc.ppre[scene], 0), n), hi = min(max(sc.ppre[scene + 1], lo), n);
    ce.start = lo;
    ce.count = hi - lo;
    ce.qx = new_xyz[(size_t)pt * 3 + 0]; ce.qy = new_xyz[(size_t)pt * 3 + 1]; ce.qz = new_xyz[(size_t)pt * 3 + 2];
    ce.row = row;
    return ce;
}

// global row of slot s, or -1 when the slot reads nothing
__device__ __forceinline__ int ssa_slot(const SsaCentre& ce, int s) {
    if (ce.row == nullptr) return -1;
    const int l = ce.row[s];
    return (l < 0 || l >= ce.count) ? -1 : ce.start + l;
}

template <int C1>
__device__ __forceinline__ float ssa_y1(const SsaCentre& ce, int g, int c, const float* __restrict__ f,
                                        const float* __restrict__ xyz, float w0, float w1, float w2, float& rx, float& ry,
                                        float& rz) {
    rx = ry = rz = 0.f;
    if (g < 0) return 0.f;
    rx = xyz[(size_t)g * 3 + 0] - ce.qx; ry = xyz[(size_t)g * 3 + 1] - ce.qy; rz = xyz[(size_t)g * 3 + 2] - ce.qz;
    return f[(size_t)g * C1 + c] + ((w0 * rx + w1 * ry) + w2 * rz);
}

// Called by every thread of the workgroup with the value of (group tid / C, channel tid % C): the groups are added in
// ascending order and partials[(q * C + channel) * gridDim.x + blockIdx.x] is written.
template <int C>
__device__ __forceinline__ void ssa_groups_to_partial(double v, double* red, double* __restrict__ partials, int q) {
    red[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x < C) {
        double a = 0.0;
        for (int j = 0; j < SSA_THREADS / C; ++j) a += red[j * C + threadIdx.x];
        partials[((size_t)q * C + threadIdx.x) * gridDim.x + blockIdx.x] = a;
    }
    __syncthreads();
}

// one 64-thread workgroup per (quantity, channel)
__global__ __launch_bounds__(64) void ssa_finish_kernel(const double* __restrict__ partials, int blocks,
                                                        double* __restrict__ sums) {
    double v[1];
    finish_partials<1>(partials + (size_t)blockIdx.x * blocks, blocks, v);
    if (threadIdx.x == 0) sums[blockIdx.x] = v[0];
}

// sums (2, C1): sum y1, sum y1^2 over the slots that read a row (every other slot has y1 = 0)
template <int C1>
__global__ __launch_bounds__(SSA_THREADS) void ssa_moments_kernel(const float* __restrict__ f, const float* __restrict__ xyz,
                                                                  const float* __restrict__ new_xyz,
                                                                  const int* __restrict__ cnt, const int* __restrict__ new_cnt,
                                                                  const int* __restrict__ idx, const float* __restrict__ w1x,
                                                                  double* __restrict__ partials, int b, int n, int m, int ns) {
    constexpr int PPB = SSA_THREADS / C1;
    __shared__ SsaScenes sc;
    __shared__ double red[SSA_THREADS];
    ssa_prefix(new_cnt, cnt, b, sc);
    __syncthreads();
    const int c = threadIdx.x % C1, grp = threadIdx.x / C1;
    const float w0 = w1x[c * 3 + 0], w1 = w1x[c * 3 + 1], w2 = w1x[c * 3 + 2];
    double sy = 0.0, syy = 0.0;
    for (int64_t pt = (int64_t)blockIdx.x * PPB + grp; pt < m; pt += (int64_t)gridDim.x * PPB) {
        const SsaCentre ce = ssa_centre(pt, m, ns, n, b, idx, new_xyz, sc);
        if (ce.row == nullptr) continue;
        for (int s = 0; s < ns; ++s) {
            float rx, ry, rz;
            const double y = (double)ssa_y1<C1>(ce, ssa_slot(ce, s), c, f, xyz, w0, w1, w2, rx, ry, rz);
            sy += y;
            syy += y * y;
        }
    }
    ssa_groups_to_partial<C1>(sy, red, partials, 0);
    ssa_groups_to_partial<C1>(syy, red, partials, 1);
}

// BWD false: u, a and the sums of y2.  BWD true (pass 1): dW2, e1 and its sums.
template <int C1, int C2, bool BWD>
__global__ __launch_bounds__(SSA_THREADS) void ssa_chain_kernel(
    const float* __restrict__ f, const float* __restrict__ xyz, const float* __restrict__ new_xyz, const int* __restrict__ cnt,
    const int* __restrict__ new_cnt, const int* __restrict__ idx, const float* __restrict__ w1x, const float* __restrict__ w2,
    const float* __restrict__ s1, const float* __restrict__ t1,
    const float* __restrict__ gamma2,                                      // fwd: its sign selects ymax or ymin
    float* __restrict__ u, uint8_t* __restrict__ arg,                      // fwd: written; pass 1: arg read
    const float* __restrict__ g, const float* __restrict__ s2, const float* __restrict__ a2, const float* __restrict__ b2,
    float* __restrict__ e1, double* __restrict__ partials, int b, int n, int m, int ns) {
    constexpr int PPB = SSA_THREADS / C2;                                  // centres per round
    constexpr int NPC = PPB * C1;                                          // (centre, c) items per round
    constexpr int IT = (NPC + SSA_THREADS - 1) / SSA_THREADS;
    __shared__ SsaScenes sc;
    __shared__ double red[SSA_THREADS];
    __shared__ __attribute__((aligned(16))) float z1s[PPB][C1];
    __shared__ float dy2s[BWD ? PPB : 1][BWD ? C2 : 1];
    __shared__ float w2s[BWD ? C2 * C1 : 1];
    ssa_prefix(new_cnt, cnt, b, sc);
    if (BWD)
        for (int e = threadIdx.x; e < C2 * C1; e += SSA_THREADS) w2s[e] = w2[e];
    __syncthreads();
    const int d = threadIdx.x % C2, grp = threadIdx.x / C2;
    const int c = threadIdx.x % C1;                                        // 256 is a multiple of C1: the same in every item
    float w2r[C1];
#pragma unroll
    for (int k = 0; k < C1; ++k) w2r[k] = w2[d * C1 + k];
    const float wx0 = w1x[c * 3 + 0], wx1 = w1x[c * 3 + 1], wx2 = w1x[c * 3 + 2], sc1 = s1[c], sh1 = t1[c];
    const bool pick_max = BWD ? true : !(gamma2[d] < 0.f);
    const float s2d = BWD ? s2[d] : 0.f, a2d = BWD ? a2[d] : 0.f, b2d = BWD ? b2[d] : 0.f;
    double sum0 = 0.0, sum1 = 0.0;                                         // fwd: y2, y2^2 of (., d); pass 1: e1, e1 y1 of (., c)
    float dw2[BWD ? C1 : 1];
    if (BWD) {
#pragma unroll
        for (int k = 0; k < C1; ++k) dw2[k] = 0.f;
    }
    for (int64_t base = (int64_t)blockIdx.x * PPB; base < m; base += (int64_t)gridDim.x * PPB) {     // uniform in the workgroup
        SsaCentre ce[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int item = (int)threadIdx.x + it * SSA_THREADS;
            ce[it] = ssa_centre(item < NPC ? base + item / C1 : (int64_t)m, m, ns, n, b, idx, new_xyz, sc);
        }
        const int64_t pt = base + grp;                                     // the centre of this thread's chain
        const bool live = pt < m;
        float ymax = 0.f, ymin = 0.f, sg = 0.f;
        int smax = 0, smin = 0, sel = -1;
        if (BWD && live) {
            sg = s2d * g[(size_t)pt * C2 + d];
            sel = (int)arg[(size_t)pt * C2 + d];
        }
        for (int s = 0; s < ns; ++s) {
            float y1v[IT];
            bool pos[IT];
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int item = (int)threadIdx.x + it * SSA_THREADS;
                y1v[it] = 0.f;
                pos[it] = false;
                if (item < NPC) {
                    float rx, ry, rz;
                    y1v[it] = ssa_y1<C1>(ce[it], ssa_slot(ce[it], s), c, f, xyz, wx0, wx1, wx2, rx, ry, rz);
                    const float z = fmaxf(sc1 * y1v[it] + sh1, 0.f);
                    pos[it] = z > 0.f;
                    z1s[item / C1][c] = z;
                }
            }
            __syncthreads();
            float y2 = 0.f;
#pragma unroll
            for (int k = 0; k < C1; k += 4) {
                const float4 z = *reinterpret_cast<const float4*>(&z1s[grp][k]);
                y2 = __builtin_fmaf(w2r[k + 0], z.x, y2);
                y2 = __builtin_fmaf(w2r[k + 1], z.y, y2);
                y2 = __builtin_fmaf(w2r[k + 2], z.z, y2);
                y2 = __builtin_fmaf(w2r[k + 3], z.w, y2);
            }
            if (!BWD) {
                if (live) {
                    sum0 += (double)y2;
                    sum1 += (double)y2 * (double)y2;
                    if (s == 0 || y2 > ymax) { ymax = y2; smax = s; }
                    if (s == 0 || y2 < ymin) { ymin = y2; smin = s; }
                }
            } else {
                float dy = 0.f;
                if (live) {
                    dy = ((s == sel) ? sg : 0.f) - a2d - b2d * y2;
#pragma unroll
                    for (int k = 0; k < C1; k += 4) {
                        const float4 z = *reinterpret_cast<const float4*>(&z1s[grp][k]);
                        dw2[k + 0] = __builtin_fmaf(dy, z.x, dw2[k + 0]);
                        dw2[k + 1] = __builtin_fmaf(dy, z.y, dw2[k + 1]);
                        dw2[k + 2] = __builtin_fmaf(dy, z.z, dw2[k + 2]);
                        dw2[k + 3] = __builtin_fmaf(dy, z.w, dw2[k + 3]);
                    }
                }
                dy2s[grp][d] = dy;
                __syncthreads();
#pragma unroll
                for (int it = 0; it < IT; ++it) {
                    const int item = (int)threadIdx.x + it * SSA_THREADS;
                    const int64_t ipt = base + item / C1;
                    if (item < NPC && ipt < m) {
                        float acc = 0.f;
#pragma unroll 8
                        for (int k = 0; k < C2; ++k) acc = __builtin_fmaf(dy2s[item / C1][k], w2s[k * C1 + c], acc);
                        const float e = pos[it] ? acc : 0.f;
                        e1[((size_t)ipt * ns + s) * C1 + c] = e;
                        sum0 += (double)e;
                        sum1 += (double)e * (double)y1v[it];
                    }
                }
            }
            __syncthreads();
        }
        if (!BWD && live) {
            u[(size_t)pt * C2 + d] = pick_max ? ymax : ymin;
            arg[(size_t)pt * C2 + d] = (uint8_t)(pick_max ? smax : smin);
        }
    }
    if (!BWD) {
        ssa_groups_to_partial<C2>(sum0, red, partials, 0);
        ssa_groups_to_partial<C2>(sum1, red, partials, 1);
    } else {
        // partials: [C1 rows of dW2^T (c, d)] then [sum e1 (C1)] [sum e1 y1 (C1)], each quantity x gridDim.x
#pragma unroll
        for (int k = 0; k < C1; ++k) ssa_groups_to_partial<C2>((double)dw2[k], red, partials, k);
        double* tail = partials + (size_t)C1 * C2 * gridDim.x;
        ssa_groups_to_partial<C1>(sum0, red, tail, 0);
        ssa_groups_to_partial<C1>(sum1, red, tail, 1);
    }
}

// pass 2: dF by atomics, partials of dW1x (3, C1)
template <int C1>
__global__ __launch_bounds__(SSA_THREADS) void ssa_bwd2_kernel(const float* __restrict__ f, const float* __restrict__ xyz,
                                                               const float* __restrict__ new_xyz, const int* __restrict__ cnt,
                                                               const int* __restrict__ new_cnt, const int* __restrict__ idx,
                                                               const float* __restrict__ w1x, const float* __restrict__ e1,
                                                               const float* __restrict__ s1, const float* __restrict__ a1,
                                                               const float* __restrict__ b1, float* __restrict__ grad_f,
                                                               double* __restrict__ partials, int b, int n, int m, int ns) {
    constexpr int PPB = SSA_THREADS / C1;
    __shared__ SsaScenes sc;
    __shared__ double red[SSA_THREADS];
    ssa_prefix(new_cnt, cnt, b, sc);
    __syncthreads();
    const int c = threadIdx.x % C1, grp = threadIdx.x / C1;
    const float w0 = w1x[c * 3 + 0], w1 = w1x[c * 3 + 1], w2 = w1x[c * 3 + 2], sc1 = s1[c], a1c = a1[c], b1c = b1[c];
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t pt = (int64_t)blockIdx.x * PPB + grp; pt < m; pt += (int64_t)gridDim.x * PPB) {
        const SsaCentre ce = ssa_centre(pt, m, ns, n, b, idx, new_xyz, sc);
        if (ce.row == nullptr) continue;               // an empty row carries no gradient
        for (int s = 0; s < ns; ++s) {
            const int row = ssa_slot(ce, s);
            if (row < 0) continue;
            float rx, ry, rz;
            const float y1 = ssa_y1<C1>(ce, row, c, f, xyz, w0, w1, w2, rx, ry, rz);
            const float dy1 = (sc1 * e1[((size_t)pt * ns + s) * C1 + c] - a1c) - b1c * y1;
            atomicAdd(grad_f + (size_t)row * C1 + c, dy1);
            v[0] += (double)dy1 * (double)rx; v[1] += (double)dy1 * (double)ry; v[2] += (double)dy1 * (double)rz;
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) ssa_groups_to_partial<C1>(v[q], red, partials, q);
}

__global__ __launch_bounds__(256) void ssa_apply_kernel(const float* __restrict__ u, const float* __restrict__ s2,
                                                        const float* __restrict__ t2, float* __restrict__ out, int64_t total,
                                                        int c2) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int d = (int)(e % c2);
        out[e] = fmaxf(s2[d] * u[e] + t2[d], 0.f);
    }
}

static bool ssa_width_ok(int c) { return c == 16 || c == 32 || c == 64; }
static bool ssa_sizes_ok(int b, int n, int m, int c1, int c2, int ns) {
    return b >= 1 && b <= SSA_MAX_B && n >= 0 && m >= 0 && ssa_width_ok(c1) && ssa_width_ok(c2) && ns >= 1 && ns <= 255 &&
           (int64_t)m * 64 <= 0x7fffffff && (int64_t)n * 64 <= 0x7fffffff;
}
static int ssa_blocks(int m, int c) {
    return (int)partial_blocks(m, SSA_THREADS / c, SSA_MAX_BLOCKS);
}

// bilinear_interpolate_torch of the reference: floor, then clamp; weights from the CLAMPED corners
struct BevCorners {
    int x0, x1, y0, y1;
    float wa, wb, wc, wd;
};
__device__ __forceinline__ BevCorners bev_corners(float x, float y, int h, int w) {
    BevCorners k;
    const float fx0 = floorf(x), fy0 = floorf(y);
    const float x0 = fminf(fmaxf(fx0, 0.f), (float)(w - 1)), x1 = fminf(fmaxf(fx0 + 1.f, 0.f), (float)(w - 1));
    const float y0 = fminf(fmaxf(fy0, 0.f), (float)(h - 1)), y1 = fminf(fmaxf(fy0 + 1.f, 0.f), (float)(h - 1));
    k.x0 = (int)x0; k.x1 = (int)x1; k.y0 = (int)y0; k.y1 = (int)y1;
    k.wa = (x1 - x) * (y1 - y);
    k.wb = (x1 - x) * (y - y0);
    k.wc = (x - x0) * (y1 - y);
    k.wd = (x - x0) * (y - y0);
    return k;
}

template <bool GRAD>
__global__ __launch_bounds__(256) void bev_interpolate_kernel(const float* __restrict__ keypoints, const float* __restrict__ xs,
                                                              const float* __restrict__ ys, const float* __restrict__ src,
                                                              float* __restrict__ dst, int64_t total, int b, int c, int h,
                                                              int w) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t pt = e / c;
        const int ch = (int)(e % c);
        const float fb = keypoints[pt * 4];
        const bool ok = fb >= 0.f && fb < (float)b && fb == floorf(fb);
        if (!ok) {
            if (!GRAD) dst[e] = 0.f;
            continue;
        }
        const BevCorners k = bev_corners(xs[pt], ys[pt], h, w);
        const size_t plane = ((size_t)(int)fb * c + ch) * h * w;
        const size_t ia = plane + (size_t)k.y0 * w + k.x0, ib = plane + (size_t)k.y1 * w + k.x0;
        const size_t ic = plane + (size_t)k.y0 * w + k.x1, id = plane + (size_t)k.y1 * w + k.x1;
        if (GRAD) {
            const float gr = src[e];
            atomicAdd(dst + ia, gr * k.wa);
            atomicAdd(dst + ib, gr * k.wb);
            atomicAdd(dst + ic, gr * k.wc);
            atomicAdd(dst + id, gr * k.wd);
        } else {
            dst[e] = ((src[ia] * k.wa + src[ib] * k.wb) + src[ic] * k.wc) + src[id] * k.wd;
        }
    }
}

static unsigned ssa_grid_for(int64_t total) {
    const int64_t blocks = divup64(total, 256);
    return (unsigned)(blocks < 65536 ? (blocks > 0 ? blocks : 1) : 65536);
}

}  // namespace pda

#define PDA_SSA_SIZES(what, b, n, m, c1, c2, ns)                                                                              \
    PDA_REQUIRE(pda::ssa_sizes_ok((b), (n), (m), (c1), (c2), (ns)),                                                             \
                what ": bad size b=%d n=%d m=%d c1=%d c2=%d (16, 32 or 64) nsample=%d (1..255)", (b), (n), (m), (c1), (c2), (ns))

// dispatch over the nine (C1, C2) pairs
#define PDA_SSA_C2(KERNEL, C1V, c2, ...)                                                                                      \
    do {                                                                                                                      \
        if ((c2) == 16) hipLaunchKernelGGL((KERNEL<C1V, 16, PDA_SSA_BWD>), __VA_ARGS__);                                        \
        else if ((c2) == 32) hipLaunchKernelGGL((KERNEL<C1V, 32, PDA_SSA_BWD>), __VA_ARGS__);                                   \
        else hipLaunchKernelGGL((KERNEL<C1V, 64, PDA_SSA_BWD>), __VA_ARGS__);                                                   \
    } while (0)
#define PDA_SSA_C1C2(KERNEL, c1, c2, ...)                                                                                     \
    do {                                                                                                                      \
        if ((c1) == 16) PDA_SSA_C2(KERNEL, 16, c2, __VA_ARGS__);                                                                \
        else if ((c1) == 32) PDA_SSA_C2(KERNEL, 32, c2, __VA_ARGS__);                                                           \
        else PDA_SSA_C2(KERNEL, 64, c2, __VA_ARGS__);                                                                           \
    } while (0)
#define PDA_SSA_C1(KERNEL, c1, ...)                                                                                           \
    do {                                                                                                                      \
        if ((c1) == 16) hipLaunchKernelGGL((KERNEL<16>), __VA_ARGS__);                                                          \
        else if ((c1) == 32) hipLaunchKernelGGL((KERNEL<32>), __VA_ARGS__);                                                     \
        else hipLaunchKernelGGL((KERNEL<64>), __VA_ARGS__);                                                                     \
    } while (0)

PDA_API int64_t pda_stack_sa_scratch_doubles(int m, int c1, int c2, int nsample) {
    if (!pda::ssa_sizes_ok(1, 0, m, c1, c2, nsample)) return -1;
    const int64_t wide = (int64_t)pda::ssa_blocks(m, c2), narrow = (int64_t)pda::ssa_blocks(m, c1);
    const int64_t pass1 = ((int64_t)c1 * c2 + 2 * c1) * wide, rest = 3 * (int64_t)c1 * narrow, fwd = 2 * (int64_t)c2 * wide;
    const int64_t a = pass1 > rest ? pass1 : rest;
    return a > fwd ? a : fwd;
}

static int ssa_zero(double* sums, int count, const char* what, pda_stream_t stream) {
    if (hipMemsetAsync(sums, 0, (size_t)count * sizeof(double), (hipStream_t)stream) != hipSuccess) return pda::check_launch(what);
    return PDA_OK;
}

PDA_API int pda_stack_sa_moments(const float* f, const float* xyz, const float* new_xyz, const int32_t* xyz_batch_cnt,
                                 const int32_t* new_xyz_batch_cnt, const int32_t* idx, const float* w1x, double* scratch,
                                 double* sums, int b, int n, int m, int c1, int nsample, pda_stream_t stream) {
    PDA_SSA_SIZES("pda_stack_sa_moments", b, n, m, c1, 16, nsample);
    PDA_REQUIRE(sums, "pda_stack_sa_moments: null pointer");
    if (m == 0 || n == 0) return ssa_zero(sums, 2 * c1, "pda_stack_sa_moments", stream);
    PDA_REQUIRE(f && xyz && new_xyz && xyz_batch_cnt && new_xyz_batch_cnt && idx && w1x && scratch,
                "pda_stack_sa_moments: null pointer");
    const int blocks = pda::ssa_blocks(m, c1);
    PDA_SSA_C1(pda::ssa_moments_kernel, c1, dim3(blocks), dim3(pda::SSA_THREADS), 0, (hipStream_t)stream, f, xyz, new_xyz,
               xyz_batch_cnt, new_xyz_batch_cnt, idx, w1x, scratch, b, n, m, nsample);
    hipLaunchKernelGGL(pda::ssa_finish_kernel, dim3(2 * c1), dim3(64), 0, (hipStream_t)stream, scratch, blocks, sums);
    return pda::check_launch("pda_stack_sa_moments");
}

PDA_API int pda_stack_sa_fwd(const float* f, const float* xyz, const float* new_xyz, const int32_t* xyz_batch_cnt,
                             const int32_t* new_xyz_batch_cnt, const int32_t* idx, const float* w1x, const float* w2,
                             const float* scale1, const float* shift1, const float* gamma2, float* u, uint8_t* arg,
                             double* scratch, double* sums, int b, int n, int m, int c1, int c2, int nsample,
                             pda_stream_t stream) {
    PDA_SSA_SIZES("pda_stack_sa_fwd", b, n, m, c1, c2, nsample);
    PDA_REQUIRE(sums, "pda_stack_sa_fwd: null pointer");
    if (m == 0) return ssa_zero(sums, 2 * c2, "pda_stack_sa_fwd", stream);
    PDA_REQUIRE(f && xyz && new_xyz && xyz_batch_cnt && new_xyz_batch_cnt && idx && w1x && w2 && scale1 && shift1 && gamma2 && u &&
                    arg && scratch,
                "pda_stack_sa_fwd: null pointer");
    const int blocks = pda::ssa_blocks(m, c2);
#define PDA_SSA_BWD false
    PDA_SSA_C1C2(pda::ssa_chain_kernel, c1, c2, dim3(blocks), dim3(pda::SSA_THREADS), 0, (hipStream_t)stream, f, xyz, new_xyz,
                 xyz_batch_cnt, new_xyz_batch_cnt, idx, w1x, w2, scale1, shift1, gamma2, u, arg, (const float*)nullptr,
                 (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, scratch, b, n, m, nsample);
#undef PDA_SSA_BWD
    hipLaunchKernelGGL(pda::ssa_finish_kernel, dim3(2 * c2), dim3(64), 0, (hipStream_t)stream, scratch, blocks, sums);
    return pda::check_launch("pda_stack_sa_fwd");
}

PDA_API int pda_stack_sa_apply(const float* u, const float* scale2, const float* shift2, float* out, int m, int c2,
                               pda_stream_t stream) {
    PDA_REQUIRE(m >= 0 && pda::ssa_width_ok(c2) && (int64_t)m * c2 <= 0x7fffffff, "pda_stack_sa_apply: bad size m=%d c2=%d", m, c2);
    if (m == 0) return PDA_OK;
    PDA_REQUIRE(u && scale2 && shift2 && out, "pda_stack_sa_apply: null pointer");
    hipLaunchKernelGGL(pda::ssa_apply_kernel, dim3(pda::ssa_grid_for((int64_t)m * c2)), dim3(256), 0, (hipStream_t)stream, u,
                       scale2, shift2, out, (int64_t)m * c2, c2);
    return pda::check_launch("pda_stack_sa_apply");
}

PDA_API int pda_stack_sa_bwd1(const float* f, const float* xyz, const float* new_xyz, const int32_t* xyz_batch_cnt,
                              const int32_t* new_xyz_batch_cnt, const int32_t* idx, const float* w1x, const float* w2,
                              const float* scale1, const float* shift1, const uint8_t* arg, const float* g, const float* scale2,
                              const float* a2, const float* b2, float* e1, double* scratch, double* sums, int b, int n, int m,
                              int c1, int c2, int nsample, pda_stream_t stream) {
    PDA_SSA_SIZES("pda_stack_sa_bwd1", b, n, m, c1, c2, nsample);
    PDA_REQUIRE(sums, "pda_stack_sa_bwd1: null pointer");
    const int count = c1 * c2 + 2 * c1;
    if (m == 0) return ssa_zero(sums, count, "pda_stack_sa_bwd1", stream);
    PDA_REQUIRE(f && xyz && new_xyz && xyz_batch_cnt && new_xyz_batch_cnt && idx && w1x && w2 && scale1 && shift1 && arg && g &&
                    scale2 && a2 && b2 && e1 && scratch,
                "pda_stack_sa_bwd1: null pointer");
    const int blocks = pda::ssa_blocks(m, c2);
#define PDA_SSA_BWD true
    PDA_SSA_C1C2(pda::ssa_chain_kernel, c1, c2, dim3(blocks), dim3(pda::SSA_THREADS), 0, (hipStream_t)stream, f, xyz, new_xyz,
                 xyz_batch_cnt, new_xyz_batch_cnt, idx, w1x, w2, scale1, shift1, (const float*)nullptr, (float*)nullptr,
                 const_cast<uint8_t*>(arg), g, scale2, a2, b2, e1, scratch, b, n, m, nsample);
#undef PDA_SSA_BWD
    hipLaunchKernelGGL(pda::ssa_finish_kernel, dim3(count), dim3(64), 0, (hipStream_t)stream, scratch, blocks, sums);
    return pda::check_launch("pda_stack_sa_bwd1");
}

PDA_API int pda_stack_sa_bwd2(const float* f, const float* xyz, const float* new_xyz, const int32_t* xyz_batch_cnt,
                              const int32_t* new_xyz_batch_cnt, const int32_t* idx, const float* w1x, const float* e1,
                              const float* scale1, const float* a1, const float* b1, float* grad_f, double* scratch,
                              double* sums, int b, int n, int m, int c1, int nsample, pda_stream_t stream) {
    PDA_SSA_SIZES("pda_stack_sa_bwd2", b, n, m, c1, 16, nsample);
    PDA_REQUIRE(sums, "pda_stack_sa_bwd2: null pointer");
    if (m == 0 || n == 0) return ssa_zero(sums, 3 * c1, "pda_stack_sa_bwd2", stream);
    PDA_REQUIRE(f && xyz && new_xyz && xyz_batch_cnt && new_xyz_batch_cnt && idx && w1x && e1 && scale1 && a1 && b1 && grad_f &&
                    scratch,
                "pda_stack_sa_bwd2: null pointer");
    const int blocks = pda::ssa_blocks(m, c1);
    PDA_SSA_C1(pda::ssa_bwd2_kernel, c1, dim3(blocks), dim3(pda::SSA_THREADS), 0, (hipStream_t)stream, f, xyz, new_xyz,
               xyz_batch_cnt, new_xyz_batch_cnt, idx, w1x, e1, scale1, a1, b1, grad_f, scratch, b, n, m, nsample);
    hipLaunchKernelGGL(pda::ssa_finish_kernel, dim3(3 * c1), dim3(64), 0, (hipStream_t)stream, scratch, blocks, sums);
    return pda::check_launch("pda_stack_sa_bwd2");
}

#define PDA_BEV_SIZES(what, m, b, c, h, w)                                                                                    \
    PDA_REQUIRE((m) >= 0 && (b) >= 1 && (c) >= 1 && (h) >= 1 && (w) >= 1 && (int64_t)(m) * (c) <= 0x7fffffff &&                   \
                    (int64_t)(b) * (c) * (h) * (w) <= 0x7fffffff,                                                             \
                what ": bad size m=%d b=%d c=%d h=%d w=%d", (m), (b), (c), (h), (w))

PDA_API int pda_bev_interpolate_fwd(const float* keypoints, const float* x_idxs, const float* y_idxs, const float* bev,
                                    float* out, int m, int b, int c, int h, int w, pda_stream_t stream) {
    PDA_BEV_SIZES("pda_bev_interpolate_fwd", m, b, c, h, w);
    if (m == 0) return PDA_OK;
    PDA_REQUIRE(keypoints && x_idxs && y_idxs && bev && out, "pda_bev_interpolate_fwd: null pointer");
    hipLaunchKernelGGL(pda::bev_interpolate_kernel<false>, dim3(pda::ssa_grid_for((int64_t)m * c)), dim3(256), 0,
                       (hipStream_t)stream, keypoints, x_idxs, y_idxs, bev, out, (int64_t)m * c, b, c, h, w);
    return pda::check_launch("pda_bev_interpolate_fwd");
}

PDA_API int pda_bev_interpolate_bwd(const float* keypoints, const float* x_idxs, const float* y_idxs, const float* grad_out,
                                    float* grad_bev, int m, int b, int c, int h, int w, pda_stream_t stream) {
    PDA_BEV_SIZES("pda_bev_interpolate_bwd", m, b, c, h, w);
    if (m == 0) return PDA_OK;
    PDA_REQUIRE(keypoints && x_idxs && y_idxs && grad_out && grad_bev, "pda_bev_interpolate_bwd: null pointer");
    hipLaunchKernelGGL(pda::bev_interpolate_kernel<true>, dim3(pda::ssa_grid_for((int64_t)m * c)), dim3(256), 0,
                       (hipStream_t)stream, keypoints, x_idxs, y_idxs, grad_out, grad_bev, (int64_t)m * c, b, c, h, w);
    return pda::check_launch("pda_bev_interpolate_bwd");
}
