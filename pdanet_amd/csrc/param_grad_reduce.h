// param_grad_reduce.h -- the fixed-order second stages that finish a parameter's gradient from per-workgroup partials:
// the split-K partials of a weight / bias gradient (csrc/wgrad.hip) and the per-block partials of LayerNorm's
// dgamma / dbeta (csrc/layer_norm.hip).  One body each, shared by the per-problem kernels and by the grouped kernel
// (pda_param_grad_reduce_grouped), so that both give the same bits: same loads, same order of additions.
#pragma once
#include "pda_common.h"

namespace pda {

// out[e] = sum_s part[s][e], fixed order.  Block = 64 elements x 16 slices of S (independent loads in groups of 8: a
// thread walking all S partials alone would serialise S load latencies).
__device__ __forceinline__ float sum_slices(const float* __restrict__ part, int S, int64_t stride, int64_t e, bool live, int slice,
                                            float (*red)[64], int el) {
    float a = 0.f;
    if (live) {
        float v[8];
        for (int s0 = slice; s0 < S; s0 += 16 * 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int sidx = s0 + 16 * u;
                v[u] = sidx < S ? part[(size_t)sidx * stride + e] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) a += v[u];
        }
    }
    red[slice][el] = a;
    __syncthreads();
    float r = 0.f;
    if (slice == 0)
#pragma unroll
        for (int p = 0; p < 16; ++p) r += red[p][el];
    __syncthreads();
    return r;
}

// Block `blk` (1024 threads) of a weight gradient's second stage: elements 64 blk .. 64 blk + 63 of dW, and of db in the
// first ceil(N / 64) blocks.  dW rows are `cols` long and `ld` floats apart in the destination (ld == cols: contiguous).
__device__ __forceinline__ void wgrad_reduce_block(const float* __restrict__ part_w, const float* __restrict__ part_b,
                                                   float* __restrict__ dw, float* __restrict__ db, int S, int64_t nm, int N,
                                                   int cols, int64_t ld, int blk, float (*red)[64]) {
    const int el = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int64_t e = (int64_t)blk * 64 + el;
    const float w = sum_slices(part_w, S, nm, e, e < nm, slice, red, el);
    if (slice == 0 && e < nm) dw[ld == cols ? e : (e / cols) * ld + e % cols] = w;
    if (db && (int64_t)blk * 64 < N) {          // block-uniform
        const float bsum = sum_slices(part_b, S, N, e, e < N, slice, red, el);
        if (slice == 0 && e < N) db[e] = bsum;
    }
}

// The same sums with 16-byte loads: block = 256 elements (64 float4 columns) x 16 slices, so a wave instruction reads 1 KB
// of one slice instead of 256 bytes and a quarter of the workgroups move the same bytes.  Per element the additions and
// their order are those of sum_slices (slice lane `slice` adds its slices in rising order, eight loads in flight; then
// the 16 lanes in order), so the bits are the same.  Needs stride, e and the element count multiples of 4 and `part`
// 16-byte aligned (wgrad_reduce_vec_ok); a float4 is inside or outside as a whole.  Returns element 256 blk + threadIdx.x
// to the first 256 threads.
__device__ __forceinline__ float sum_slices4(const float* __restrict__ part, int S, int64_t stride, int64_t e4, bool live, int slice,
                                             float (*red)[256], int q) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
        float4 v[8];
        for (int s0 = slice; s0 < S; s0 += 16 * 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int sidx = s0 + 16 * u;
                v[u] = sidx < S ? *reinterpret_cast<const float4*>(part + (size_t)sidx * stride + e4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w; }
        }
    }
    *reinterpret_cast<float4*>(&red[slice][4 * q]) = a;
    __syncthreads();
    float r = 0.f;
    if (threadIdx.x < 256)
#pragma unroll
        for (int p = 0; p < 16; ++p) r += red[p][threadIdx.x];
    __syncthreads();
    return r;
}

__host__ __device__ __forceinline__ bool wgrad_reduce_vec_ok(const float* part_w, const float* part_b, int64_t nm, int N) {
    return (nm & 3) == 0 && (N & 3) == 0 && (((uintptr_t)part_w | (uintptr_t)part_b) & 15) == 0;
}

// wgrad_reduce_block on 256 elements per block: blocks = ceil(nm / 256), db in the first ceil(N / 256) of them
__device__ __forceinline__ void wgrad_reduce_block4(const float* __restrict__ part_w, const float* __restrict__ part_b,
                                                    float* __restrict__ dw, float* __restrict__ db, int S, int64_t nm, int N,
                                                    int cols, int64_t ld, int blk, float (*red)[256]) {
    const int q = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int64_t e4 = (int64_t)blk * 256 + 4 * q, e = (int64_t)blk * 256 + threadIdx.x;
    const float w = sum_slices4(part_w, S, nm, e4, e4 < nm, slice, red, q);
    if (threadIdx.x < 256 && e < nm) dw[ld == cols ? e : (e / cols) * ld + e % cols] = w;
    if (db && (int64_t)blk * 256 < N) {         // block-uniform
        const float bsum = sum_slices4(part_b, S, N, e4, e4 < N, slice, red, q);
        if (threadIdx.x < 256 && e < N) db[e] = bsum;
    }
}

// Block `blk` (1024 threads) of LayerNorm's second stage: dbeta / dgamma = sum of the [nblocks][2][d] per-block partials;
// 64 columns x 16 slices per block.
__device__ __forceinline__ void layer_norm_finalize_block(const float* __restrict__ partial, int nblocks, int d,
                                                          float* __restrict__ dgamma, float* __restrict__ dbeta, int blk,
                                                          float (*red)[16][64]) {
    const int cl = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int c = blk * 64 + cl;
    float a = 0.f, b = 0.f;
    if (c < d) {
        float va[8], vb[8];
        for (int k0 = part; k0 < nblocks; k0 += 16 * 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + 16 * u;
                va[u] = k < nblocks ? partial[((size_t)k * 2 + 0) * d + c] : 0.f;
                vb[u] = k < nblocks ? partial[((size_t)k * 2 + 1) * d + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { a += va[u]; b += vb[u]; }
        }
    }
    red[0][part][cl] = a; red[1][part][cl] = b;
    __syncthreads();
    if (part != 0 || c >= d) return;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int p = 0; p < 16; ++p) { s1 += red[0][p][cl]; s2 += red[1][p][cl]; }
    dbeta[c] = s1;
    dgamma[c] = s2;
}

// pda_param_grad_entry_t::kind (include/pda_train.h)
constexpr int PARAM_GRAD_WEIGHT = 0, PARAM_GRAD_LAYER_NORM = 1;

}  // namespace pda
