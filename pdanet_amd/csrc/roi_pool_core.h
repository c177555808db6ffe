// roi_pool_core.h -- the device functions of the RoI-aware pooling that roi_pool.hip (roiaware_pool3d, one scene a call) and
// parta2.hip (the Part-A2 head's input stage, all scenes and both poolings in one pass) share: the voxel index expression,
// the walk that collects a box's points into the slots of its voxels, and the max, avg and gradient steps over those slots.
//
// The walk: a workgroup owns a box and goes over rows [p_begin, p_end) of the points in ascending 256-point tiles: every lane
// tests one point (box_rec.h, the trigonometry done once), the tile's hits are compacted in point order with ballots and a
// prefix over the four waves, and every hit finds its slot as (points its voxel already holds) + (earlier hits of the same
// voxel in this tile), so slots 1..count hold the first K-1 points of a voxel in ascending row whatever order the lanes run
// in.  No mask, no atomics.  The stored value is the row itself, so a caller that walks a segment of a stacked point set
// keeps GLOBAL rows.
#pragma once
#include "pda_common.h"
#include "box_rec.h"

namespace pda {

constexpr int ROI_TILE = 256;
constexpr int ROI_LDS_VOX = 4096;                  // 16 KB of counters: up to 16^3 voxels

__device__ __forceinline__ uint64_t lanes_below() { return (1ull << lane_id()) - 1ull; }

// the reference's index expression (roiaware_pool3d_kernel.cu:60-70): float32 operations, truncation, UNSIGNED clamp
// (a negative index lands in the last voxel)
__device__ __forceinline__ int roi_voxel_axis(float local, float d, int out) {
    const float res = d / (float)out;
    const unsigned int idx = (unsigned int)(int)((local + d / 2) / res);
    return (int)min(idx, (unsigned int)(out - 1));
}

// exclusive prefix of this wave over the workgroup's four ballot counts, and their total
__device__ __forceinline__ int roi_wave_prefix(const int* wave_cnt, int wave, int& total) {
    int off = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < ROI_TILE / 64; ++w) {
        const int c = wave_cnt[w];
        off += w < wave ? c : 0;
        sum += c;
    }
    total = sum;
    return off;
}

// b: the box row (7 floats).  xyz: the x of point row 0, rows `stride` floats apart.  mine: the box's (n_vox, k_slots) table.
// LDS_CNT: the voxel counters live in cnt[n_vox] (LDS) and reach slot 0 at the end -- only where they are not zero (the
// caller zero-filled the table) or, with ALL_COUNTS, everywhere (the table needs no fill: no slot past a count is ever read).
// Without LDS_CNT slot 0 of the zero-filled table is the counter.  Called by all 256 threads of the workgroup.
template <bool LDS_CNT, bool ALL_COUNTS>
__device__ __forceinline__ void roi_collect_walk(const float* __restrict__ b, const float* __restrict__ xyz, int stride, int p_begin,
                                                 int p_end, int* __restrict__ mine, int out_x, int out_y, int out_z, int k_slots,
                                                 int* cnt, int* hit_vox, int (*wave_cnt)[ROI_TILE / 64]) {
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const float dx = b[3], dy = b[4], dz = b[5];
    const BoxRec rec = make_box_rec(b[0], b[1], b[2], dx, dy, dz, b[6], (double)1e-5f);
    const int n_vox = out_x * out_y * out_z, cap = k_slots - 1;
    if (LDS_CNT) {
        for (int v = tid; v < n_vox; v += ROI_TILE) cnt[v] = 0;
    }
    __syncthreads();
    int it = 0;
    for (int t0 = p_begin; t0 < p_end; t0 += ROI_TILE, it ^= 1) {
        const int pt = t0 + tid;
        bool hit = false;
        int vox = 0;
        if (pt < p_end) {
            const float* p = xyz + (size_t)pt * stride;
            const float x = p[0], y = p[1], z = p[2];
            float lx = 0.f, ly = 0.f;
            hit = in_box_rec_local<PDA_FP_CONTRACT != 0>(rec, x, y, z, lx, ly);
            if (hit) {
                const int xi = roi_voxel_axis(lx, dx, out_x), yi = roi_voxel_axis(ly, dy, out_y);
                const int zi = roi_voxel_axis(z - rec.cz, dz, out_z);
                vox = (xi * out_y + yi) * out_z + zi;
            }
        }
        const uint64_t mask = __ballot(hit);
        if (lane == 0) wave_cnt[it][wave] = __popcll(mask);
        __syncthreads();                           // wave_cnt[it] is next written two tiles on, behind the next barrier
        int n_hits;
        const int pos = roi_wave_prefix(wave_cnt[it], wave, n_hits) + __popcll(mask & lanes_below());
        if (n_hits == 0) continue;                 // workgroup-uniform
        if (hit) hit_vox[pos] = vox;
        __syncthreads();
        int rank = 0, total = 0, base = 0;
        if (hit) {
            for (int j = 0; j < n_hits; ++j) {
                const int same = hit_vox[j] == vox;
                rank += same & (int)(j < pos);
                total += same;
            }
            base = LDS_CNT ? cnt[vox] : mine[(size_t)vox * k_slots];
        }
        __syncthreads();                           // every counter is read before any is moved
        if (hit) {
            const int slot = base + rank;
            if (slot < cap) mine[(size_t)vox * k_slots + 1 + slot] = pt;
            if (rank == 0) {
                const int moved = min(base + total, cap);
                if (LDS_CNT) cnt[vox] = moved;
                else mine[(size_t)vox * k_slots] = moved;
            }
        }
        // the next tile reads the counters behind its own two barriers; hit_vox is rewritten behind its first
    }
    if (LDS_CNT) {
        __syncthreads();
        for (int v = tid; v < n_vox; v += ROI_TILE) {
            const int c = cnt[v];
            if (ALL_COUNTS || c > 0) mine[(size_t)v * k_slots] = c;
        }
    }
}

// total order of the non-NaN floats as signed integers, -0 == +0 (the files are built with -fno-honor-nans, so the strict
// `>` that NaN must lose is not left to a float compare)
__device__ __forceinline__ int roi_order_key(uint32_t bits) {
    if (bits == 0x80000000u) bits = 0u;
    return (int)(bits ^ ((uint32_t)((int)bits >> 31) & 0x7fffffffu));
}

// the largest feat[p][ch] over slots 1..n of idx (ties keep the lower slot; NaN, -inf and rows outside [0, pts_num) never
// win): its row, or -1, and its bits
__device__ __forceinline__ int roi_slot_max(const float* __restrict__ feat, const int* __restrict__ idx, int n, int pts_num,
                                            int channels, int ch, uint32_t& best_bits) {
    int best_key = roi_order_key(0xff800000u), arg = -1;      // -inf: strict > never takes -inf itself
    best_bits = 0;
    for (int k = 1; k <= n; ++k) {
        const int p = idx[k];
        if (p < 0 || p >= pts_num) continue;
        const uint32_t bits = __float_as_uint(feat[(size_t)p * channels + ch]);
        const bool is_nan = (bits & 0x7fffffffu) > 0x7f800000u;
        const int key = roi_order_key(bits);
        if (!is_nan && key > best_key) { best_key = key; best_bits = bits; arg = p; }
    }
    return arg;
}

// the float32 sum of read(p) over slots 1..n of idx in slot order; the average is this over (float)n
template <typename Read>
__device__ __forceinline__ float roi_slot_sum(const int* __restrict__ idx, int n, int pts_num, Read read) {
    float sum = 0.f;
    for (int k = 1; k <= n; ++k) {
        const int p = idx[k];
        if (p < 0 || p >= pts_num) continue;
        sum += read(p);
    }
    return sum;
}

// the average's gradient: add(p, grad / max(n, 1)) for every slot
template <typename Add>
__device__ __forceinline__ void roi_slot_avg_grad(const int* __restrict__ idx, int n, int pts_num, float grad_out, Add add) {
    const float g = grad_out * (1 / fmaxf((float)n, 1.0f));
    for (int k = 1; k <= n; ++k) {
        const int p = idx[k];
        if (p < 0 || p >= pts_num) continue;
        add(p, g);
    }
}

// a voxel's count as the pooling reads it
__device__ __forceinline__ int roi_slot_count(int c, int k_slots) { return min(max(c, 0), k_slots - 1); }

// the max pooling's gradient, called by every thread of a 256-wide grid: grad_in[argmax[e], e % channels] += grad_out[e]
__device__ __forceinline__ void roi_max_grad(const int* __restrict__ argmax, const float* __restrict__ grad_out,
                                             float* __restrict__ grad_in, int pts_num, int channels, size_t total) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int p = argmax[e];
        if (p < 0 || p >= pts_num) continue;
        atomicAdd(grad_in + (size_t)p * channels + e % channels, grad_out[e]);
    }
}

}  // namespace pda
