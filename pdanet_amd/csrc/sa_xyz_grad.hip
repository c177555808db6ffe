// sa_xyz_grad.hip -- the COORDINATE columns of the first layer of a vanilla set-abstraction scale in the backward pass
// (include/pda_train.h).  z1 = [xyz[idx] - new_xyz | features[idx]] W1^T with W1 (c1, 3 + C) (QueryAndGroup + the first
// 1x1 convolution, pointnet2_utils.py:671-704 + pointnet2_modules.py:1657).  Its backward splits by column block:
//   * the C feature columns are a plain (tokens x C) problem: weight gradient on csrc/wgrad.hip, input gradient on
//     csrc/gemm_split.hip, both at full matrix-core width (C = 256);
//   * the 3 coordinate columns made the whole thing a 259-wide problem that went to the library.  Here they are one
//     streaming pass over grad_z1 (thread = output channel, tokens in order): dW1[:, 0:3] += g (x) (xyz[idx] - centre)
//     and, per centre, grad_new_xyz = -(sum over its samples of g) W1[:, 0:3] -- the centre enters every sample with -1.
// The pass reads grad_z1 once (tokens * c1 * 4 bytes) and nothing else of size.
#include "pda_common.h"

namespace pda {

constexpr int XG_BLOCKS = 512;
constexpr int XG_THREADS = 256;
constexpr int XG_MAXC = 4;      // channels per thread: c1 <= 1024

template <int CPT>
__global__ __launch_bounds__(XG_THREADS) void sa_xyz_grad_kernel(const float* __restrict__ g, const float* __restrict__ xyz,
                                                                 const float* __restrict__ new_xyz, const int32_t* __restrict__ idx,
                                                                 const float* __restrict__ w, int ldw, float* __restrict__ partial,
                                                                 float* __restrict__ grad_new, int n, int m, int ns, int c1, int64_t groups) {
    __shared__ float red[XG_THREADS / 64][3];
    const int tid = threadIdx.x;
    float accw[CPT][3], wx[CPT][3];
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
        const int o = tid + q * XG_THREADS;
#pragma unroll
        for (int d = 0; d < 3; ++d) { accw[q][d] = 0.f; wx[q][d] = o < c1 ? w[(size_t)o * ldw + d] : 0.f; }
    }
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int bs = (int)(grp / m);
        const float* ct = new_xyz + grp * 3;
        const float cx = ct[0], cy = ct[1], cz = ct[2];
        const float* pts = xyz + (size_t)bs * n * 3;
        const int32_t* ids = idx + grp * ns;
        const float* grow = g + grp * ns * (int64_t)c1;
        float gs[CPT];
#pragma unroll
        for (int q = 0; q < CPT; ++q) gs[q] = 0.f;
        for (int s0 = 0; s0 < ns; s0 += 8) {
            float gv[8][CPT], dx[8], dy[8], dz[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int s = s0 + u < ns ? s0 + u : ns - 1;
                const float* pt = pts + (size_t)ids[s] * 3;
                dx[u] = pt[0] - cx; dy[u] = pt[1] - cy; dz[u] = pt[2] - cz;          // pointnet2_utils.py:692
#pragma unroll
                for (int q = 0; q < CPT; ++q) {
                    const int o = tid + q * XG_THREADS;
                    gv[u][q] = (s0 + u < ns && o < c1) ? grow[(int64_t)s * c1 + o] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int q = 0; q < CPT; ++q) {
                    accw[q][0] = __builtin_fmaf(gv[u][q], dx[u], accw[q][0]);
                    accw[q][1] = __builtin_fmaf(gv[u][q], dy[u], accw[q][1]);
                    accw[q][2] = __builtin_fmaf(gv[u][q], dz[u], accw[q][2]);
                    gs[q] += gv[u][q];
                }
        }
        if (grad_new) {
            float v[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < CPT; ++q)
#pragma unroll
                for (int d = 0; d < 3; ++d) v[d] = __builtin_fmaf(gs[q], wx[q][d], v[d]);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) v[d] += __shfl_xor(v[d], o);
            }
            __syncthreads();                     // the previous group's result has been read
            if (lane_id() == 0) { red[wave_id()][0] = v[0]; red[wave_id()][1] = v[1]; red[wave_id()][2] = v[2]; }
            __syncthreads();
            if (tid < 3) grad_new[grp * 3 + tid] = -((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]));
        }
    }
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
        const int o = tid + q * XG_THREADS;
        if (o < c1) {
            float* p = partial + ((size_t)blockIdx.x * c1 + o) * 3;
            p[0] = accw[q][0]; p[1] = accw[q][1]; p[2] = accw[q][2];
        }
    }
}

// 16 elements x 16 slices of the workgroup partials per block, slices summed in fixed order
__global__ __launch_bounds__(256) void sa_xyz_grad_reduce_kernel(const float* __restrict__ partial, int nblocks, int c1, float* __restrict__ dw, int lddw) {
    __shared__ double red[16][16];
    const int el = threadIdx.x & 15, part = threadIdx.x >> 4;
    const int e = blockIdx.x * 16 + el;
    const bool ok = e < c1 * 3;
    double a = 0.0;
    if (ok)
        for (int k = part; k < nblocks; k += 16) a += (double)partial[(size_t)k * c1 * 3 + e];
    red[part][el] = a;
    __syncthreads();
    if (part == 0 && ok) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) t += red[q][el];
        dw[(size_t)(e / 3) * lddw + e % 3] = (float)t;
    }
}

// ---- forward: the first layer of a wide SA scale WITHOUT a per-token contraction ------------------------------------------
// z1[token] = W1 [xyz[idx] - centre | f[idx]] = (W_f f)[idx] + W_xyz (xyz[idx] - centre): a linear layer commutes with the
// gather.  The feature part is computed once per POINT (P = F W_f^T: b*n rows instead of b*m*nsample -- 4096 instead of
// 229 376 at ONCE layer 5: 0.5 GFLOP instead of 30) and gathered as rows here; the coordinate part is three FMAs per
// output on the centred coordinates themselves (no cancellation between large absolute coordinates).
// thread = 4 consecutive channels of one token; P rows (c1 floats) are L2-resident (4 MB), z1 leaves as 16-byte stores.
// STATS (training): the thread also keeps the sum and the sum of squares of what it stores, in double, for its four channels; the
// 256 / (c1/4) threads of the workgroup that share a channel quad are added through LDS in thread order and the workgroup
// writes ONE row partial[block][2][c1] -- the layout pda_bn_finalize_fwd reads (the statistics pass over z1 is gone).
template <bool STATS>
__global__ __launch_bounds__(256) void sa_point_gather_kernel(const float* __restrict__ prow, const float* __restrict__ xyz,
                                                              const float* __restrict__ new_xyz, const int32_t* __restrict__ idx,
                                                              const float* __restrict__ w, int ldw, const float* __restrict__ bias,
                                                              int relu, float* __restrict__ z, int n, int m, int ns, int c1,
                                                              int64_t tokens, double* __restrict__ partial) {
    const int cq = c1 >> 2;                                         // channel quads per token
    // cq divides 256 (c1 in {128, 256, 512, 1024}: the launcher checks): a thread keeps ONE channel quad for the whole walk, so
    // its 12 coordinate weights are loaded once (per token they would be 12 loads at a 1 KB stride across the wave)
    const int q = threadIdx.x % cq;
    float wx[4], wy[4], wz[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float* wr = w + (size_t)(4 * q + k) * ldw;             // W1 row of this channel: columns 0..2 are the coordinates'
        wx[k] = wr[0]; wy[k] = wr[1]; wz[k] = wr[2];
    }
    float bq[4] = {0.f, 0.f, 0.f, 0.f};                             // inference: the folded BatchNorm shift, then ReLU
    if (bias) { const float4 b4 = *reinterpret_cast<const float4*>(bias + 4 * q); bq[0] = b4.x; bq[1] = b4.y; bq[2] = b4.z; bq[3] = b4.w; }
    const int tpb = 256 / cq;                                        // tokens per workgroup step
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    for (int64_t tok = (int64_t)blockIdx.x * tpb + threadIdx.x / cq; tok < tokens; tok += (int64_t)gridDim.x * tpb) {
        const int64_t grp = tok / ns;
        const int bs = (int)(grp / m);
        const int id = idx[tok];
        const float* pt = xyz + ((size_t)bs * n + id) * 3;
        const float* ct = new_xyz + grp * 3;
        const float dx = pt[0] - ct[0], dy = pt[1] - ct[1], dz = pt[2] - ct[2];      // pointnet2_utils.py:692
        const float4 p4 = *reinterpret_cast<const float4*>(prow + ((size_t)bs * n + id) * c1 + 4 * q);
        const float pv[4] = {p4.x, p4.y, p4.z, p4.w};
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k] = __builtin_fmaf(wz[k], dz, __builtin_fmaf(wy[k], dy, __builtin_fmaf(wx[k], dx, pv[k]))) + bq[k];
            o[k] = relu ? fmaxf(o[k], 0.f) : o[k];
        }
        *reinterpret_cast<float4*>(z + tok * c1 + 4 * q) = make_float4(o[0], o[1], o[2], o[3]);
        if constexpr (STATS) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { s1[k] += (double)o[k]; s2[k] += (double)o[k] * (double)o[k]; }
        }
    }
    if constexpr (STATS) {
        __shared__ double lds[2 * 256 * 4];
        double* la = lds;
        double* lb = lds + 256 * 4;
        const int tid = threadIdx.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) { la[tid * 4 + k] = s1[k]; lb[tid * 4 + k] = s2[k]; }
        __syncthreads();
        if (tid < cq) {                                              // tid == its channel quad: rows r = 0 .. tpb-1 in order
            double a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
            for (int r = 0; r < tpb; ++r)
#pragma unroll
                for (int k = 0; k < 4; ++k) { a[k] += la[(r * cq + tid) * 4 + k]; b[k] += lb[(r * cq + tid) * 4 + k]; }
            double* pa = partial + (size_t)blockIdx.x * 2 * c1;
#pragma unroll
            for (int k = 0; k < 4; ++k) { pa[4 * tid + k] = a[k]; pa[c1 + 4 * tid + k] = b[k]; }
        }
    }
}

// ---- backward of the same layer behind a training-mode BatchNorm + ReLU, in ONE pass ----------------------------------------
// sa_xyz_grad_kernel's walk (thread = channel, a workgroup takes whole groups in token order) with the gradient at z1 FORMED here
// from the gradient at relu(bn(z1)) -- bn_apply_kernel<true>'s expression (csrc/bn_relu.hip), the channel's constants in
// registers -- instead of read: gz1 is never written.  While the value is in a register it goes three ways: the coordinate
// columns of dW1 and the centre's gradient exactly as in sa_xyz_grad_kernel, and the scatter-add onto the point the token was
// gathered from (one float per lane: a wave's atomic instruction adds 256 contiguous bytes of one point row, the full-rate shape
// of csrc/group_gather.hip).  Consecutive tokens of a group with the same neighbour (ball-query padding repeats one to the end of
// the list) are added in the register and leave as ONE atomic.
// Grid cap, measured on ONCE layer 5 (three scales, ms per step, this kernel + the second stage over its partials): 512 workgroups
// 0.220 + 0.037, 1024: 0.209 + 0.066, 2048: 0.221 + 0.124 -- the kernel runs at the rate of its atomics either way and the second
// stage grows with the partials.
constexpr int PG_BLOCKS = 512;

template <int CPT>
__global__ __launch_bounds__(XG_THREADS) void sa_point_grad_bn_kernel(const float* __restrict__ ga, const float* __restrict__ z,
                                                                      const float* __restrict__ mean_invstd, const float* __restrict__ gamma,
                                                                      const float* __restrict__ beta, const float* __restrict__ sums,
                                                                      const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                                      const int32_t* __restrict__ idx, const float* __restrict__ w, int ldw,
                                                                      float* __restrict__ partial, float* __restrict__ grad_new,
                                                                      float* __restrict__ g_pts, int n, int m, int ns, int c1, int64_t groups) {
    __shared__ float red[XG_THREADS / 64][3];
    const int tid = threadIdx.x;
    float accw[CPT][3], wx[CPT][3], mu[CPT], is[CPT], gm[CPT], be[CPT], m1[CPT], m2[CPT];
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
        const int o = tid + q * XG_THREADS;
        const bool ok = o < c1;
#pragma unroll
        for (int d = 0; d < 3; ++d) { accw[q][d] = 0.f; wx[q][d] = ok ? w[(size_t)o * ldw + d] : 0.f; }
        mu[q] = ok ? mean_invstd[o] : 0.f; is[q] = ok ? mean_invstd[c1 + o] : 0.f;
        gm[q] = ok ? gamma[o] : 0.f; be[q] = ok ? beta[o] : 0.f;
        m1[q] = ok ? sums[o] : 0.f; m2[q] = ok ? sums[c1 + o] : 0.f;
    }
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int bs = (int)(grp / m);
        const float* ct = new_xyz + grp * 3;
        const float cx = ct[0], cy = ct[1], cz = ct[2];
        const float* pts = xyz + (size_t)bs * n * 3;
        const int32_t* ids = idx + grp * ns;
        const float* grow = ga + grp * ns * (int64_t)c1;
        const float* zrow = z + grp * ns * (int64_t)c1;
        float* prow = g_pts + (size_t)bs * n * c1;
        float gs[CPT], run[CPT];
#pragma unroll
        for (int q = 0; q < CPT; ++q) { gs[q] = 0.f; run[q] = 0.f; }
        int run_id = -1;                          // the neighbour whose gradients are being added up in `run`
        auto flush = [&]() {
            if ((unsigned)run_id < (unsigned)n) {
#pragma unroll
                for (int q = 0; q < CPT; ++q) {
                    const int o = tid + q * XG_THREADS;
                    if (o < c1) atomicAdd(prow + (size_t)run_id * c1 + o, run[q]);
                }
            }
        };
        for (int s0 = 0; s0 < ns; s0 += 8) {
            float gv[8][CPT], zv[8][CPT], dx[8], dy[8], dz[8];
            int id[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int s = s0 + u < ns ? s0 + u : ns - 1;
                id[u] = ids[s];
                const float* pt = pts + (size_t)id[u] * 3;
                dx[u] = pt[0] - cx; dy[u] = pt[1] - cy; dz[u] = pt[2] - cz;          // pointnet2_utils.py:692
#pragma unroll
                for (int q = 0; q < CPT; ++q) {
                    const int o = tid + q * XG_THREADS;
                    const bool ok = s0 + u < ns && o < c1;
                    gv[u][q] = ok ? grow[(int64_t)s * c1 + o] : 0.f;
                    zv[u][q] = ok ? zrow[(int64_t)s * c1 + o] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bool live = s0 + u < ns;
                float gz[CPT];
#pragma unroll
                for (int q = 0; q < CPT; ++q) {
                    const int o = tid + q * XG_THREADS;
                    const float wgt = 1.f;                                           // bn_apply_kernel<true> with unit row weights
                    const float xh = (zv[u][q] - mu[q]) * is[q];
                    const float dyh = (xh * gm[q] + be[q] > 0.f) ? gv[u][q] : 0.f;
                    const float v = gm[q] * is[q] * (dyh - wgt * (m1[q] + xh * m2[q]));
                    gz[q] = (live && o < c1) ? v : 0.f;
                    accw[q][0] = __builtin_fmaf(gz[q], dx[u], accw[q][0]);
                    accw[q][1] = __builtin_fmaf(gz[q], dy[u], accw[q][1]);
                    accw[q][2] = __builtin_fmaf(gz[q], dz[u], accw[q][2]);
                    gs[q] += gz[q];
                }
                if (live) {                                                          // uniform over the workgroup, as is id[u]
                    if (id[u] == run_id) {
#pragma unroll
                        for (int q = 0; q < CPT; ++q) run[q] += gz[q];
                    } else {
                        flush();
                        run_id = id[u];
#pragma unroll
                        for (int q = 0; q < CPT; ++q) run[q] = gz[q];
                    }
                }
            }
        }
        flush();
        if (grad_new) {
            float v[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < CPT; ++q)
#pragma unroll
                for (int d = 0; d < 3; ++d) v[d] = __builtin_fmaf(gs[q], wx[q][d], v[d]);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) v[d] += __shfl_xor(v[d], o);
            }
            __syncthreads();                     // the previous group's result has been read
            if (lane_id() == 0) { red[wave_id()][0] = v[0]; red[wave_id()][1] = v[1]; red[wave_id()][2] = v[2]; }
            __syncthreads();
            if (tid < 3) grad_new[grp * 3 + tid] = -((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]));
        }
    }
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
        const int o = tid + q * XG_THREADS;
        if (o < c1) {
            float* p = partial + ((size_t)blockIdx.x * c1 + o) * 3;
            p[0] = accw[q][0]; p[1] = accw[q][1]; p[2] = accw[q][2];
        }
    }
}

// The statistics variant's grid: one row of 2 * c1 doubles per workgroup goes to pda_bn_finalize_fwd, so the plain gather's 8192
// workgroups would mean 32 MB of partials at c1 = 256.  Measured on ONCE layer 5 (three scales, ms per step, gather + all of the
// step's finalize launches): cap 512: 0.113 + 0.257, 1024: 0.086 + 0.268, 2048: 0.094 + 0.294, 4096: 0.100 + 0.343.
constexpr int PG_STATS_BLOCKS = 1024;

static int gather_blocks(int64_t tokens, int c1, int cap) {
    const int64_t steps = divup64(tokens * (c1 >> 2), 256);
    return (int)(steps < cap ? steps : cap);
}

static int launch_point_gather(const float* point_rows, const float* xyz, const float* new_xyz, const int32_t* idx, const float* w, int ldw,
                               const float* bias, int relu, float* z, double* partial, bool stats, int b, int n, int m, int ns, int c1,
                               hipStream_t stream, const char* what) {
    PDA_REQUIRE(b >= 0 && n >= 1 && m >= 0 && ns >= 1 && c1 >= 4 && (c1 & 3) == 0 && ldw >= 3, "%s: bad size", what);
    const int64_t tokens = (int64_t)b * m * ns;
    if (tokens == 0) return PDA_OK;
    PDA_REQUIRE(point_rows && xyz && new_xyz && idx && w && z && (((uintptr_t)point_rows | (uintptr_t)z | (uintptr_t)bias) & 15) == 0,
                "%s: null or misaligned pointer", what);
    PDA_REQUIRE(!stats || (partial && ((uintptr_t)partial & 7) == 0), "%s: null or misaligned partial", what);
    if (256 % (c1 >> 2) != 0) {
        set_error("%s: c1 = %d (c1 / 4 must divide 256)", what, c1);
        return PDA_ERR_UNSUPPORTED;
    }
    if (stats)
        hipLaunchKernelGGL(sa_point_gather_kernel<true>, dim3(gather_blocks(tokens, c1, PG_STATS_BLOCKS)), dim3(256), 0, stream, point_rows, xyz,
                           new_xyz, idx, w, ldw, bias, relu, z, n, m, ns, c1, tokens, partial);
    else
        hipLaunchKernelGGL(sa_point_gather_kernel<false>, dim3(gather_blocks(tokens, c1, 8192)), dim3(256), 0, stream, point_rows, xyz, new_xyz,
                           idx, w, ldw, bias, relu, z, n, m, ns, c1, tokens, (double*)nullptr);
    return check_launch(what);
}

}  // namespace pda

PDA_API int pda_sa_point_gather(const float* point_rows, const float* xyz, const float* new_xyz, const int32_t* idx, const float* w, int ldw,
                                const float* bias, int relu, float* z, int b, int n, int m, int ns, int c1, pda_stream_t stream) {
    return pda::launch_point_gather(point_rows, xyz, new_xyz, idx, w, ldw, bias, relu, z, nullptr, false, b, n, m, ns, c1, (hipStream_t)stream,
                                    "pda_sa_point_gather");
}

PDA_API int64_t pda_sa_point_gather_stats_blocks(int64_t tokens, int c1) {
    return tokens > 0 && c1 >= 4 ? pda::gather_blocks(tokens, c1, pda::PG_STATS_BLOCKS) : 0;
}

PDA_API int pda_sa_point_gather_stats(const float* point_rows, const float* xyz, const float* new_xyz, const int32_t* idx, const float* w,
                                      int ldw, float* z, double* partial, int b, int n, int m, int ns, int c1, pda_stream_t stream) {
    return pda::launch_point_gather(point_rows, xyz, new_xyz, idx, w, ldw, nullptr, 0, z, partial, true, b, n, m, ns, c1, (hipStream_t)stream,
                                    "pda_sa_point_gather_stats");
}

PDA_API int64_t pda_sa_xyz_grad_scratch_bytes(int c1) {
    constexpr int blocks = pda::XG_BLOCKS > pda::PG_BLOCKS ? pda::XG_BLOCKS : pda::PG_BLOCKS;
    return c1 > 0 ? (int64_t)blocks * c1 * 3 * sizeof(float) : 0;
}

PDA_API int pda_sa_point_grad_bn(const float* grad_a1, const float* z1, const float* mean_invstd, const float* gamma, const float* beta,
                                 const float* bwd_sums, const float* xyz, const float* new_xyz, const int32_t* idx, const float* w, int ldw,
                                 float* dw, int lddw, float* grad_new_xyz, float* grad_points, void* scratch, int b, int n, int m, int ns,
                                 int c1, pda_stream_t stream) {
    using namespace pda;
    PDA_REQUIRE(b >= 0 && n >= 1 && m >= 0 && ns >= 1 && c1 >= 1 && ldw >= 3 && lddw >= 3, "pda_sa_point_grad_bn: bad size");
    PDA_REQUIRE(grad_points || (int64_t)b * c1 == 0, "pda_sa_point_grad_bn: null pointer");
    const hipStream_t s = (hipStream_t)stream;
    if ((int64_t)b * c1 > 0) {
        // the kernel ADDS onto the points: cleared here, on the stream, instead of by a fill kernel of the caller's
        const hipError_t e = hipMemsetAsync(grad_points, 0, (size_t)b * n * c1 * sizeof(float), s);
        PDA_REQUIRE(e == hipSuccess, "pda_sa_point_grad_bn: hipMemsetAsync: %s", hipGetErrorString(e));
    }
    const int64_t groups = (int64_t)b * m;
    if (groups == 0) return PDA_OK;
    PDA_REQUIRE(grad_a1 && z1 && mean_invstd && gamma && beta && bwd_sums && xyz && new_xyz && idx && w && dw && scratch,
                "pda_sa_point_grad_bn: null pointer");
    if (c1 > XG_THREADS * XG_MAXC) {
        set_error("pda_sa_point_grad_bn: c1 = %d > %d", c1, XG_THREADS * XG_MAXC);
        return PDA_ERR_UNSUPPORTED;
    }
    const int blocks = (int)(groups < PG_BLOCKS ? groups : PG_BLOCKS);
    float* partial = (float*)scratch;
    const int cpt = divup(c1, XG_THREADS);
#define PDA_PG(CPT) hipLaunchKernelGGL((sa_point_grad_bn_kernel<CPT>), dim3(blocks), dim3(XG_THREADS), 0, s, grad_a1, z1, mean_invstd, gamma, beta, \
                                       bwd_sums, xyz, new_xyz, idx, w, ldw, partial, grad_new_xyz, grad_points, n, m, ns, c1, groups)
    if (cpt == 1) PDA_PG(1); else if (cpt == 2) PDA_PG(2); else PDA_PG(4);
#undef PDA_PG
    hipLaunchKernelGGL(sa_xyz_grad_reduce_kernel, dim3(divup(c1 * 3, 16)), dim3(256), 0, s, (const float*)partial, blocks, c1, dw, lddw);
    return check_launch("pda_sa_point_grad_bn");
}

PDA_API int pda_sa_xyz_grad(const float* grad_z1, const float* xyz, const float* new_xyz, const int32_t* idx, const float* w, int ldw,
                            float* dw, int lddw, float* grad_new_xyz, void* scratch, int b, int n, int m, int ns, int c1,
                            pda_stream_t stream) {
    using namespace pda;
    PDA_REQUIRE(b >= 0 && n >= 1 && m >= 0 && ns >= 1 && c1 >= 1 && ldw >= 3 && lddw >= 3, "pda_sa_xyz_grad: bad size");
    const int64_t groups = (int64_t)b * m;
    if (groups == 0) return PDA_OK;
    PDA_REQUIRE(grad_z1 && xyz && new_xyz && idx && w && dw && scratch, "pda_sa_xyz_grad: null pointer");
    if (c1 > XG_THREADS * XG_MAXC) {
        set_error("pda_sa_xyz_grad: c1 = %d > %d", c1, XG_THREADS * XG_MAXC);
        return PDA_ERR_UNSUPPORTED;
    }
    const hipStream_t s = (hipStream_t)stream;
    const int blocks = (int)(groups < XG_BLOCKS ? groups : XG_BLOCKS);
    float* partial = (float*)scratch;
    const int cpt = divup(c1, XG_THREADS);
#define PDA_XG(CPT) hipLaunchKernelGGL((sa_xyz_grad_kernel<CPT>), dim3(blocks), dim3(XG_THREADS), 0, s, grad_z1, xyz, new_xyz, idx, w, ldw, \
                                       partial, grad_new_xyz, n, m, ns, c1, groups)
    if (cpt == 1) PDA_XG(1); else if (cpt == 2) PDA_XG(2); else PDA_XG(4);
#undef PDA_XG
    hipLaunchKernelGGL(sa_xyz_grad_reduce_kernel, dim3(divup(c1 * 3, 16)), dim3(256), 0, s, (const float*)partial, blocks, c1, dw, lddw);
    return check_launch("pda_sa_xyz_grad");
}
