// loss_sums.h -- float64 sums of a loss over a grid, added in ONE fixed order so that a loss value does not depend on the
// schedule: every thread keeps N running sums; block_sums_to_partials reduces them to partials (N, gridDim.x); one
// 64-thread workgroup finishes with finish_partials.  The order of additions: xor butterfly 32 -> 1 inside a wave, lane 0
// of each wave to LDS, thread q adds the waves of quantity q in ascending order; in the finish lane i adds partials[i],
// partials[i + 64], ..., then the butterfly.  (head_loss.hip's hl_block_sum is a different contract: the result in every
// thread, its LDS reused inside one kernel.)
#pragma once
#include "pda_common.h"

namespace pda {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Called once, by every thread of a THREADS-wide workgroup: partials[q * gridDim.x + blockIdx.x] = the block's sum of v[q].
template <int N, int THREADS>
__device__ __forceinline__ void block_sums_to_partials(const double (&v)[N], double* __restrict__ partials) {
    __shared__ double red[N][THREADS / 64];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    double s[N];      // all butterflies first: independent chains the scheduler interleaves
#pragma unroll
    for (int q = 0; q < N; ++q) s[q] = wave_sum_f64(v[q]);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q) red[q][wave] = s[q];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double a = 0.0;
        for (int w = 0; w < THREADS / 64; ++w) a += red[threadIdx.x][w];
        partials[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = a;
    }
}

// Called by the 64 threads of the finishing workgroup: v[q] = the sum of partials[q * blocks ..], in every lane.
template <int N>
__device__ __forceinline__ void finish_partials(const double* __restrict__ partials, int blocks, double (&v)[N]) {
    for (int q = 0; q < N; ++q) {
        double a = 0.0;
        for (int i = threadIdx.x; i < blocks; i += 64) a += partials[(size_t)q * blocks + i];
        v[q] = wave_sum_f64(a);
    }
}

// The grid of the first pass: one workgroup per `per_block` elements, at most `cap` (the kernels stride over the rest).
inline int64_t partial_blocks(int64_t n, int64_t per_block, int64_t cap) {
    if (n <= 0) return 0;
    const int64_t blocks = divup64(n, per_block);
    return blocks < cap ? blocks : cap;
}

}  // namespace pda
