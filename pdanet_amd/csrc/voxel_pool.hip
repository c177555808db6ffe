// voxel_pool.hip -- the RoI-grid pooling of Voxel R-CNN, one scale of NeighborVoxelSAModuleMSG (voxel_pool_modules.py:86-121
// of the reference) after mlps_in, without its (1, C, M, nsample) intermediates: grouped features, position conv, its
// BatchNorm, the sum, the ReLU.  The query stays pda_stack_voxel_query (stack_pool.hip); idx is its output as it stands.
//
// A slot (i, s) reads row g = idx[i][s] of xyz and features_in.  It reads NOTHING, and stands for rel = 0, f = 0, when the row
// is empty (idx[i][0] < 0, the query's mark) or g lies outside [0, n): vp_row is the one statement of that rule.
//
// Value of a slot, float32, in this order and without contraction (the file is built with -ffp-contract=off):
//     p = (w0 * rx + w1 * ry) + w2 * rz        rel = xyz[g] - new_xyz[i], the float32 difference
//     v = max((f + scale * p) + shift, 0)
// out = the largest v of the row, arg = the first slot that attains it (strict > while walking s upwards).
//
// BatchNorm2d's batch statistics of y = W rel over all M * nsample slots follow from nine sums of rel (y is linear in a
// 3-vector): voxel_pool_moments leaves them in float64; Python derives scale / shift from them (voxel_pool_modules.py).
// The backward needs, per channel, sum g, sum g p*, sum g rel* over the winners (g = grad_out where out > 0): the same
// per-workgroup partials and fixed-order finish (loss_sums.h).  Only grad_features_in is added with float atomics, as in
// the stacked grouping backward (stack_ops.hip); that sum is not bit-reproducible.
//
// Layout: a group of C lanes per grid point, lane = channel.  A slot's feature row is one coalesced 128- or 256-byte read,
// idx / xyz / new_xyz are uniform over the group, and the atomics of a group cover one contiguous row segment.
#include "loss_sums.h"

namespace pda {

constexpr int VP_THREADS = 256;
constexpr int VP_SLOTS_PER_BLOCK = 2048;     // moments: (i, s) slots per workgroup
constexpr int VP_POINTS_PER_LANE = 8;        // backward: grid points per lane before the grid is capped
constexpr int VP_MAX_BLOCKS = 1024;

__device__ __forceinline__ int vp_row(int g, bool empty, int n) { return (empty || g < 0 || g >= n) ? -1 : g; }

__device__ __forceinline__ float vp_pos(float w0, float w1, float w2, float rx, float ry, float rz) {
    return (w0 * rx + w1 * ry) + w2 * rz;
}

__global__ __launch_bounds__(VP_THREADS) void voxel_pool_moments_kernel(const int* __restrict__ idx,
                                                                        const float* __restrict__ xyz,
                                                                        const float* __restrict__ new_xyz, int n,
                                                                        int64_t total, int ns, double* __restrict__ partials) {
    double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t e = (int64_t)blockIdx.x * VP_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * VP_THREADS) {
        const int64_t i = e / ns;
        const int g = vp_row(idx[e], idx[i * ns] < 0, n);
        if (g < 0) continue;                       // rel = 0 adds nothing to any sum
        const double x = (double)(xyz[(size_t)g * 3 + 0] - new_xyz[i * 3 + 0]);
        const double y = (double)(xyz[(size_t)g * 3 + 1] - new_xyz[i * 3 + 1]);
        const double z = (double)(xyz[(size_t)g * 3 + 2] - new_xyz[i * 3 + 2]);
        v[0] += x; v[1] += y; v[2] += z;
        v[3] += x * x; v[4] += x * y; v[5] += x * z; v[6] += y * y; v[7] += y * z; v[8] += z * z;
    }
    block_sums_to_partials<9, VP_THREADS>(v, partials);
}

__global__ __launch_bounds__(64) void voxel_pool_moments_finish_kernel(const double* __restrict__ partials, int blocks,
                                                                       double* __restrict__ sums) {
    double v[9];
    finish_partials<9>(partials, blocks, v);
#pragma unroll
    for (int q = 0; q < 9; ++q)
        if (threadIdx.x == q) sums[q] = v[q];
}

template <int C>
__global__ __launch_bounds__(VP_THREADS) void voxel_pool_fwd_kernel(const float* __restrict__ feat, const int* __restrict__ idx,
                                                                    const float* __restrict__ xyz,
                                                                    const float* __restrict__ new_xyz,
                                                                    const float* __restrict__ w, const float* __restrict__ scale,
                                                                    const float* __restrict__ shift, float* __restrict__ out,
                                                                    uint8_t* __restrict__ arg, int n, int m, int ns) {
    const int c = threadIdx.x % C;
    const int pt = blockIdx.x * (VP_THREADS / C) + threadIdx.x / C;
    if (pt >= m) return;
    const float w0 = w[c * 3 + 0], w1 = w[c * 3 + 1], w2 = w[c * 3 + 2], sc = scale[c], sh = shift[c];
    const float qx = new_xyz[(size_t)pt * 3 + 0], qy = new_xyz[(size_t)pt * 3 + 1], qz = new_xyz[(size_t)pt * 3 + 2];
    const int* row = idx + (size_t)pt * ns;
    const int g0 = row[0];
    const bool empty = g0 < 0;
    const int slots = empty ? 1 : ns;              // every slot of an empty row has slot 0's value
    float best = 0.f;
    int best_s = 0;
    for (int s = 0; s < slots; ++s) {
        const int gi = row[s];
        if (s > 0 && gi == g0) continue;           // the query pads with its first hit: slot 0's value again, never a winner
        const int g = vp_row(gi, empty, n);
        float rx = 0.f, ry = 0.f, rz = 0.f, f = 0.f;
        if (g >= 0) {
            rx = xyz[(size_t)g * 3 + 0] - qx; ry = xyz[(size_t)g * 3 + 1] - qy; rz = xyz[(size_t)g * 3 + 2] - qz;
            f = feat[(size_t)g * C + c];
        }
        const float v = fmaxf((f + sc * vp_pos(w0, w1, w2, rx, ry, rz)) + sh, 0.f);
        if (s == 0 || v > best) { best = v; best_s = s; }
    }
    out[(size_t)pt * C + c] = best;
    arg[(size_t)pt * C + c] = (uint8_t)best_s;
}

template <int C>
__global__ __launch_bounds__(VP_THREADS) void voxel_pool_bwd_kernel(const float* __restrict__ grad_out,
                                                                    const float* __restrict__ out,
                                                                    const uint8_t* __restrict__ arg, const int* __restrict__ idx,
                                                                    const float* __restrict__ xyz,
                                                                    const float* __restrict__ new_xyz,
                                                                    const float* __restrict__ w, float* __restrict__ grad_feat,
                                                                    double* __restrict__ partials, int n, int m, int ns) {
    constexpr int PPB = VP_THREADS / C;
    __shared__ double red[5][VP_THREADS];
    const int c = threadIdx.x % C, sub = threadIdx.x / C;
    const float w0 = w[c * 3 + 0], w1 = w[c * 3 + 1], w2 = w[c * 3 + 2];
    double v[5] = {0, 0, 0, 0, 0};
    for (int64_t pt = (int64_t)blockIdx.x * PPB + sub; pt < m; pt += (int64_t)gridDim.x * PPB) {
        const size_t o = (size_t)pt * C + c;
        if (!(out[o] > 0.f)) continue;             // the ReLU's mask
        const float g = grad_out[o];
        const int* row = idx + (size_t)pt * ns;
        const int s = min((int)arg[o], ns - 1);    // arg is an input: never past the row
        const int r = vp_row(row[s], row[0] < 0, n);
        float rx = 0.f, ry = 0.f, rz = 0.f;
        if (r >= 0) {
            rx = xyz[(size_t)r * 3 + 0] - new_xyz[(size_t)pt * 3 + 0];
            ry = xyz[(size_t)r * 3 + 1] - new_xyz[(size_t)pt * 3 + 1];
            rz = xyz[(size_t)r * 3 + 2] - new_xyz[(size_t)pt * 3 + 2];
            atomicAdd(grad_feat + (size_t)r * C + c, g);
        }
        const double dg = (double)g;
        v[0] += dg;
        v[1] += dg * (double)vp_pos(w0, w1, w2, rx, ry, rz);
        v[2] += dg * (double)rx; v[3] += dg * (double)ry; v[4] += dg * (double)rz;
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) red[q][threadIdx.x] = v[q];
    __syncthreads();
    if (threadIdx.x < C) {                         // the point groups of the workgroup in ascending order
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double a = 0.0;
            for (int j = 0; j < PPB; ++j) a += red[q][j * C + c];
            partials[((size_t)q * C + c) * gridDim.x + blockIdx.x] = a;
        }
    }
}

// one 64-thread workgroup per (quantity, channel)
__global__ __launch_bounds__(64) void voxel_pool_bwd_finish_kernel(const double* __restrict__ partials, int blocks,
                                                                   double* __restrict__ sums) {
    double v[1];
    finish_partials<1>(partials + (size_t)blockIdx.x * blocks, blocks, v);
    if (threadIdx.x == 0) sums[blockIdx.x] = v[0];
}

static int vp_moment_blocks(int m, int ns) {
    return (int)partial_blocks((int64_t)m * ns, VP_SLOTS_PER_BLOCK, VP_MAX_BLOCKS);
}
static int vp_bwd_blocks(int m, int c) {
    return (int)partial_blocks(m, (int64_t)(VP_THREADS / c) * VP_POINTS_PER_LANE, VP_MAX_BLOCKS);
}
static bool vp_sizes_ok(int m, int c, int ns) { return m >= 0 && (c == 32 || c == 64) && ns >= 1 && ns <= 255; }

}  // namespace pda

#define PDA_VP_SIZES(what, n, m, c, ns)                                                                                       \
    PDA_REQUIRE((n) >= 0 && pda::vp_sizes_ok((m), (c), (ns)) && (int64_t)(m) * (c) <= 0x7fffffff,                               \
                what ": bad size n=%d m=%d c=%d (32 or 64) nsample=%d (1..255)", (n), (m), (c), (ns))

PDA_API int64_t pda_voxel_pool_scratch_doubles(int m, int c, int nsample) {
    if (!pda::vp_sizes_ok(m, c, nsample)) return -1;
    const int64_t a = 9 * (int64_t)pda::vp_moment_blocks(m, nsample), b = 5 * (int64_t)c * pda::vp_bwd_blocks(m, c);
    return a > b ? a : b;
}

PDA_API int pda_voxel_pool_moments(const int32_t* idx, const float* xyz, const float* new_xyz, double* scratch, double* sums,
                                   int n, int m, int nsample, pda_stream_t stream) {
    PDA_VP_SIZES("pda_voxel_pool_moments", n, m, 32, nsample);
    PDA_REQUIRE(sums, "pda_voxel_pool_moments: null pointer");
    if (m == 0) {
        if (hipMemsetAsync(sums, 0, 9 * sizeof(double), (hipStream_t)stream) != hipSuccess)
            return pda::check_launch("pda_voxel_pool_moments");
        return PDA_OK;
    }
    PDA_REQUIRE(idx && xyz && new_xyz && scratch, "pda_voxel_pool_moments: null pointer");
    const int blocks = pda::vp_moment_blocks(m, nsample);
    hipLaunchKernelGGL(pda::voxel_pool_moments_kernel, dim3(blocks), dim3(pda::VP_THREADS), 0, (hipStream_t)stream, idx, xyz,
                       new_xyz, n, (int64_t)m * nsample, nsample, scratch);
    hipLaunchKernelGGL(pda::voxel_pool_moments_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scratch, blocks, sums);
    return pda::check_launch("pda_voxel_pool_moments");
}

PDA_API int pda_voxel_pool_fwd(const float* features_in, const int32_t* idx, const float* xyz, const float* new_xyz,
                               const float* w, const float* scale, const float* shift, float* out, uint8_t* arg, int n, int m,
                               int c, int nsample, pda_stream_t stream) {
    PDA_VP_SIZES("pda_voxel_pool_fwd", n, m, c, nsample);
    if (m == 0) return PDA_OK;
    PDA_REQUIRE(features_in && idx && xyz && new_xyz && w && scale && shift && out && arg, "pda_voxel_pool_fwd: null pointer");
    const dim3 grid(pda::divup(m, pda::VP_THREADS / c)), block(pda::VP_THREADS);
    if (c == 32)
        hipLaunchKernelGGL(pda::voxel_pool_fwd_kernel<32>, grid, block, 0, (hipStream_t)stream, features_in, idx, xyz, new_xyz, w,
                           scale, shift, out, arg, n, m, nsample);
    else
        hipLaunchKernelGGL(pda::voxel_pool_fwd_kernel<64>, grid, block, 0, (hipStream_t)stream, features_in, idx, xyz, new_xyz, w,
                           scale, shift, out, arg, n, m, nsample);
    return pda::check_launch("pda_voxel_pool_fwd");
}

PDA_API int pda_voxel_pool_bwd(const float* grad_out, const float* out, const uint8_t* arg, const int32_t* idx, const float* xyz,
                               const float* new_xyz, const float* w, float* grad_features_in, double* scratch, double* sums,
                               int n, int m, int c, int nsample, pda_stream_t stream) {
    PDA_VP_SIZES("pda_voxel_pool_bwd", n, m, c, nsample);
    PDA_REQUIRE(sums, "pda_voxel_pool_bwd: null pointer");
    if (m == 0) {
        if (hipMemsetAsync(sums, 0, 5 * (size_t)c * sizeof(double), (hipStream_t)stream) != hipSuccess)
            return pda::check_launch("pda_voxel_pool_bwd");
        return PDA_OK;
    }
    PDA_REQUIRE(grad_out && out && arg && idx && xyz && new_xyz && w && grad_features_in && scratch,
                "pda_voxel_pool_bwd: null pointer");
    const int blocks = pda::vp_bwd_blocks(m, c);
    const dim3 grid(blocks), block(pda::VP_THREADS);
    if (c == 32)
        hipLaunchKernelGGL(pda::voxel_pool_bwd_kernel<32>, grid, block, 0, (hipStream_t)stream, grad_out, out, arg, idx, xyz,
                           new_xyz, w, grad_features_in, scratch, n, m, nsample);
    else
        hipLaunchKernelGGL(pda::voxel_pool_bwd_kernel<64>, grid, block, 0, (hipStream_t)stream, grad_out, out, arg, idx, xyz,
                           new_xyz, w, grad_features_in, scratch, n, m, nsample);
    hipLaunchKernelGGL(pda::voxel_pool_bwd_finish_kernel, dim3(5 * c), dim3(64), 0, (hipStream_t)stream, scratch, blocks, sums);
    return pda::check_launch("pda_voxel_pool_bwd");
}
