// radix_sort.h -- the stable 8-bit LSD radix sort of (key, value) pairs and the tile counts and scans around it, shared by
// dyn_voxel.hip (which describes the passes) and sparse_conv_index.hip.  The live pair count is read on the device
// (counts[0], clipped to n), every grid depends on n alone, and the only atomics are LDS integer adds into a histogram.
#pragma once
#include "pda_common.h"

namespace pda {
namespace {

constexpr int DV_TILE = 256;                      // threads of every workgroup but the scan's; rows of a compaction tile
constexpr int DV_WAVES = DV_TILE / PDA_WAVE;
constexpr int DV_ITEMS = 8;                       // pairs a thread handles in a sort tile
constexpr int DV_SORT_TILE = DV_TILE * DV_ITEMS;
constexpr int DV_RADIX = 256;

static_assert(DV_RADIX == DV_TILE, "thread t owns digit t");

__device__ __forceinline__ int live(const int32_t* __restrict__ counts, int which, int64_t cap) {
    const int32_t v = counts[which];
    return v < 0 ? 0 : (v > cap ? (int)cap : v);      // a caller's buffer is never left, whatever counts holds
}

// Sums a flag over the workgroup's tile of DV_TILE threads and stores it.
__device__ __forceinline__ void store_tile_count(bool f, int32_t* __restrict__ o) {
    __shared__ int32_t wc[DV_WAVES];
    const uint64_t bal = __ballot(f);
    if (lane_id() == 0) wc[wave_id()] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t s = 0;
        for (int w = 0; w < DV_WAVES; ++w) s += wc[w];
        *o = s;
    }
}

// Flagged threads of the tile up to and including this one (every thread of the workgroup calls this).
__device__ __forceinline__ int tile_rank_inclusive(bool f) {
    __shared__ int32_t wc[DV_WAVES];
    const uint64_t bal = __ballot(f);
    const int w = wave_id();
    if (lane_id() == 0) wc[w] = __popcll(bal);
    __syncthreads();
    int pos = rank_below(bal) + (f ? 1 : 0);
    for (int v = 0; v < w; ++v) pos += wc[v];
    return pos;
}

// The exclusive scan of a[0 .. m) in place by one workgroup of THREADS threads; thread u owns `per` consecutive entries.
// Returns the total (valid in every thread).
template <int THREADS>
__device__ __forceinline__ int32_t block_scan(int32_t* __restrict__ a, int m) {
    __shared__ int32_t part[THREADS];
    const int u = threadIdx.x;
    const int per = (m + THREADS - 1) / THREADS;
    const int t0 = min(m, u * per), t1 = min(m, t0 + per);
    int32_t s = 0;
    for (int t = t0; t < t1; ++t) s += a[t];
    part[u] = s;
    __syncthreads();
    for (int o = 1; o < THREADS; o <<= 1) {          // Hillis-Steele inclusive scan of the partial sums
        const int32_t v = u >= o ? part[u - o] : 0;
        __syncthreads();
        part[u] += v;
        __syncthreads();
    }
    int32_t run = part[u] - s;
    for (int t = t0; t < t1; ++t) {
        const int32_t c = a[t];
        a[t] = run;
        run += c;
    }
    return part[THREADS - 1];
}

// One workgroup: the tile counts of a compaction; the total goes to *total.
__global__ __launch_bounds__(1024) void dv_scan(int32_t* __restrict__ a, int m, int32_t* __restrict__ total) {
    const int32_t sum = block_scan<1024>(a, m);
    if (threadIdx.x == 0) *total = sum;
}

// One workgroup per digit: the scan of the digit's row of tile counts, and the row's total.
__global__ __launch_bounds__(DV_TILE) void dv_scan_digit(int32_t* __restrict__ hist, int tiles, int32_t* __restrict__ digit_total) {
    const int32_t sum = block_scan<DV_TILE>(hist + (int64_t)blockIdx.x * tiles, tiles);
    if (threadIdx.x == 0) digit_total[blockIdx.x] = sum;
}

// ---- the sort ----------------------------------------------------------------------------------------------------------
// hist[d * tiles + t] = the pairs of sort tile t whose digit is d.
__global__ __launch_bounds__(DV_TILE) void dv_digit_count(int n, int shift, int tiles, const int32_t* __restrict__ counts,
                                                          const uint32_t* __restrict__ key, int32_t* __restrict__ hist) {
    __shared__ int32_t h[DV_RADIX];
    const int t = blockIdx.x, u = threadIdx.x;
    const int nk = live(counts, 0, n);
    h[u] = 0;
    __syncthreads();
    for (int r = 0; r < DV_ITEMS; ++r) {
        const int64_t j = (int64_t)t * DV_SORT_TILE + r * DV_TILE + u;
        if (j < nk) atomicAdd(&h[(key[j] >> shift) & (DV_RADIX - 1)], 1);
    }
    __syncthreads();
    hist[(int64_t)u * tiles + t] = h[u];
}

// A pair goes to base[digit] (the scanned histogram) + the pairs of its tile with the same digit in front of it: those of
// earlier rounds (folded into base after every round), of earlier waves of this round (wc) and of lower lanes of this wave.
__global__ __launch_bounds__(DV_TILE) void dv_digit_scatter(int n, int shift, int tiles, const int32_t* __restrict__ counts,
                                                            const int32_t* __restrict__ hist,
                                                            const int32_t* __restrict__ digit_total,
                                                            const uint32_t* __restrict__ key, const int32_t* __restrict__ val,
                                                            uint32_t* __restrict__ key_out, int32_t* __restrict__ val_out) {
    __shared__ int32_t base[DV_RADIX], wc[DV_WAVES][DV_RADIX];
    const int t = blockIdx.x, u = threadIdx.x, w = wave_id();
    const int nk = live(counts, 0, n);
    const int32_t total = digit_total[u];
    base[u] = total;
#pragma unroll
    for (int v = 0; v < DV_WAVES; ++v) wc[v][u] = 0;
    __syncthreads();
    for (int o = 1; o < DV_RADIX; o <<= 1) {          // the pairs of all lower digits: the inclusive scan of the totals ...
        const int32_t v = u >= o ? base[u - o] : 0;
        __syncthreads();
        base[u] += v;
        __syncthreads();
    }
    base[u] += hist[(int64_t)u * tiles + t] - total;      // ... made exclusive, plus this digit's pairs in earlier tiles
    __syncthreads();
    for (int r = 0; r < DV_ITEMS; ++r) {
        const int64_t j = (int64_t)t * DV_SORT_TILE + r * DV_TILE + u;
        const bool valid = j < nk;
        const uint32_t k = valid ? key[j] : 0u;
        const int32_t x = valid ? val[j] : 0;
        const uint32_t d = (k >> shift) & (DV_RADIX - 1);
        uint64_t same = __ballot(valid);                       // the valid lanes of this wave with my digit
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1u;
            const uint64_t b = __ballot(one);
            same &= one ? b : ~b;
        }
        const int below = rank_below(same);
        if (valid && below == 0) wc[w][d] = __popcll(same);
        __syncthreads();
        if (valid) {
            int pos = base[d] + below;
            for (int v = 0; v < w; ++v) pos += wc[v][d];
            if (pos < nk) {                                    // always, for a histogram of these very keys
                key_out[pos] = k;
                val_out[pos] = x;
            }
        }
        __syncthreads();
        int32_t s = 0;
#pragma unroll
        for (int v = 0; v < DV_WAVES; ++v) {
            s += wc[v][u];
            wc[v][u] = 0;
        }
        base[u] += s;
        __syncthreads();
    }
}

int64_t sort_tiles_of(int64_t n) { return divup64(n, DV_SORT_TILE); }

// The sort of the live pairs of (key[cur], val[cur]) by the low `key_bits` bits; returns the index of the buffers that hold
// the result.  hist: sort_tiles_of(n) * DV_RADIX int32, digit_total: DV_RADIX int32.
inline int radix_sort_pairs(int n, int key_bits, const int32_t* counts, uint32_t* const key[2], int32_t* const val[2], int32_t* hist,
                            int32_t* digit_total, hipStream_t st) {
    const int stiles = (int)sort_tiles_of(n), passes = (key_bits + 7) / 8;
    const dim3 sgrid((unsigned)stiles), block(DV_TILE);
    int cur = 0;
    for (int p = 0; p < passes; ++p, cur ^= 1) {
        hipLaunchKernelGGL(dv_digit_count, sgrid, block, 0, st, n, 8 * p, stiles, counts, key[cur], hist);
        hipLaunchKernelGGL(dv_scan_digit, dim3(DV_RADIX), block, 0, st, hist, stiles, digit_total);
        hipLaunchKernelGGL(dv_digit_scatter, sgrid, block, 0, st, n, 8 * p, stiles, counts, hist, digit_total, key[cur], val[cur],
                           key[cur ^ 1], val[cur ^ 1]);
    }
    return cur;
}

}  // namespace
}  // namespace pda
