// input_stage.hip -- the input stage of the data loader on the device (include/pda_train.h, pda_input_stage /
// pda_input_boxes): B ragged raw scenes -> the collated (B * num_points, 1 + C) batch the detector takes.
//
// Per scene it reproduces the reference's chain DataProcessor.mask_points_and_boxes_outside_range -> sample_points ->
// shuffle_points (pcdet/datasets/processor/data_processor.py) followed by DatasetTemplate.collate_batch:
//   masked  = the points with lo <= x <= hi and lo <= y <= hi (z is not tested), in their original order;
//   near    = sqrt((x*x + y*y) + z*z) < 40 (np.linalg.norm over float32: uncontracted, this order, correctly rounded);
//   n = |masked|, n_far = |masked and not near|, k = num_points:
//     (A) n > k, n_far < k : r = k - n_far near points without replacement, then every far point in order;
//     (B) n > k, n_far >= k: k masked points without replacement;
//     (C) n <= k           : every masked point in order, then k - n draws with replacement;
//   then sample_points' shuffle (perm1) and, when enabled, shuffle_points (perm2):
//     out[j] = choice[perm1[perm2[j]]]  (perm2 = identity when shuffle_points is off).
// The launches are sized from B and n_cap only, so nothing is read back to the host:
//   is_count_kernel   (tiles, B): masked / near counts per tile of 256 points;
//   is_scan_kernel    (B)       : exclusive scan of the tile counts in place, scene totals and status into info;
//   is_scatter_kernel (tiles, B): stable compaction -- mlist = masked points, plist = near points then far points
//                                 (scene-local raw indices), positions from 64-bit ballots + mbcnt;
//   is_output_kernel  (k/256, B): one thread per output row resolves its source through the permutations and the case,
//                                 then writes [b, x, y, z, features...].
// The draws come from the caller (explicit mode: pick / perm1 / perm2 as int32 (B, k)) or from a 64-bit seed (seeded
// mode): a keyed bijection on [0, m) -- a 6-round Feistel network over 2h bits (4^h >= m) with cycle walking -- gives
// the samples without replacement (its first r outputs) and the shuffles; a counter-based hash gives case C's draws.
#include "pda_common.h"
#include "ragged_scene.h"
#include "stage_rng.h"

namespace pda {
namespace {

constexpr int IS_TILE = 256;
constexpr int IS_WAVES = IS_TILE / PDA_WAVE;
// info[b][3] status bits of this stage (include/pda_train.h), next to ragged_scene.h's
constexpr int ST_EMPTY = 1, ST_BAD_DRAW = 8;

struct Range {
    float lo[3], hi[3];
};

__device__ __forceinline__ bool in_range_xy(float x, float y, const Range& rg) {
    return x >= rg.lo[0] && x <= rg.hi[0] && y >= rg.lo[1] && y <= rg.hi[1];
}

// The file is built with -ffp-contract=off: no FMA here.  __builtin_sqrtf lowers to the correctly rounded sequence
// (HIP's default -fhip-fp32-correctly-rounded-divide-sqrt).
__device__ __forceinline__ bool is_near(float x, float y, float z) {
    return __builtin_sqrtf((x * x + y * y) + z * z) < 40.0f;
}

__device__ __forceinline__ void point_flags(const float* __restrict__ pts, const Scene& s, int i, int c, const Range& rg,
                                            bool& masked, bool& near) {
    masked = near = false;
    if (i < s.n) {
        const float* p = pts + (s.start + i) * (int64_t)c;
        const float x = p[0], y = p[1], z = p[2];
        masked = in_range_xy(x, y, rg);
        near = masked && is_near(x, y, z);
    }
}

// ---- kernels ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IS_TILE) void is_count_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off,
                                                           int64_t n_total, int c, int64_t n_cap, Range rg, int tiles,
                                                           int32_t* __restrict__ tile_cnt) {
    __shared__ int32_t wm[IS_WAVES], wn[IS_WAVES];
    const int b = blockIdx.y, t = blockIdx.x;
    const Scene s = scene_of(off, b, n_total, n_cap);
    bool masked, near;
    point_flags(pts, s, t * IS_TILE + (int)threadIdx.x, c, rg, masked, near);
    const uint64_t bm = __ballot(masked), bn = __ballot(near);
    if (lane_id() == 0) {
        wm[wave_id()] = __popcll(bm);
        wn[wave_id()] = __popcll(bn);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t sm = 0, sn = 0;
        for (int w = 0; w < IS_WAVES; ++w) { sm += wm[w]; sn += wn[w]; }
        int32_t* o = tile_cnt + ((int64_t)b * tiles + t) * 2;
        o[0] = sm;
        o[1] = sn;
    }
}

// One workgroup per scene.  Thread u owns the `per` consecutive tiles from u * per.
__global__ __launch_bounds__(1024) void is_scan_kernel(const int64_t* __restrict__ off, int64_t n_total, int64_t n_cap,
                                                       int tiles, int32_t* __restrict__ tile_cnt, int32_t* __restrict__ info) {
    __shared__ int32_t pm[1024], pn[1024];
    const int b = blockIdx.x, u = threadIdx.x;
    const int per = (tiles + 1023) / 1024;
    const int t0 = min(tiles, u * per), t1 = min(tiles, t0 + per);
    int32_t* tc = tile_cnt + (int64_t)b * tiles * 2;
    int32_t sm = 0, sn = 0;
    for (int t = t0; t < t1; ++t) { sm += tc[2 * t]; sn += tc[2 * t + 1]; }
    pm[u] = sm;
    pn[u] = sn;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {          // Hillis-Steele inclusive scan of the 1024 partial sums
        const int32_t vm = u >= o ? pm[u - o] : 0, vn = u >= o ? pn[u - o] : 0;
        __syncthreads();
        pm[u] += vm;
        pn[u] += vn;
        __syncthreads();
    }
    int32_t rm = pm[u] - sm, rn = pn[u] - sn;
    for (int t = t0; t < t1; ++t) {
        const int32_t cm = tc[2 * t], cn = tc[2 * t + 1];
        tc[2 * t] = rm;
        tc[2 * t + 1] = rn;
        rm += cm;
        rn += cn;
    }
    if (u == 1023) {
        const Scene s = scene_of(off, b, n_total, n_cap);
        const int32_t n = pm[1023], n_near = pn[1023];
        info[b * 4 + 0] = n;
        info[b * 4 + 1] = n - n_near;
        info[b * 4 + 3] = s.status | (n == 0 ? ST_EMPTY : 0);
    }
}

__global__ __launch_bounds__(IS_TILE) void is_scatter_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off,
                                                             int64_t n_total, int c, int64_t n_cap, Range rg, int tiles,
                                                             const int32_t* __restrict__ tile_off, const int32_t* __restrict__ info,
                                                             int32_t* __restrict__ mlist, int32_t* __restrict__ plist) {
    __shared__ int32_t wm[IS_WAVES], wn[IS_WAVES];
    const int b = blockIdx.y, t = blockIdx.x;
    const Scene s = scene_of(off, b, n_total, n_cap);
    const int i = t * IS_TILE + (int)threadIdx.x;
    bool masked, near;
    point_flags(pts, s, i, c, rg, masked, near);
    const uint64_t bm = __ballot(masked), bn = __ballot(near);
    const int w = wave_id();
    if (lane_id() == 0) {
        wm[w] = __popcll(bm);
        wn[w] = __popcll(bn);
    }
    __syncthreads();
    if (!masked) return;
    const int32_t* to = tile_off + ((int64_t)b * tiles + t) * 2;
    int32_t pos_m = to[0] + rank_below(bm), pos_n = to[1] + rank_below(bn);
    for (int v = 0; v < w; ++v) { pos_m += wm[v]; pos_n += wn[v]; }
    const int32_t n_near = info[b * 4 + 0] - info[b * 4 + 1];
    const int64_t base = (int64_t)b * n_cap;
    mlist[base + pos_m] = i;
    // masked points before me minus near points before me = far points before me
    plist[base + (near ? pos_n : n_near + (pos_m - pos_n))] = i;
}

struct Draws {
    const int32_t* pick;   // explicit mode, (B, k) each; NULL in seeded mode
    const int32_t* perm1;
    const int32_t* perm2;  // NULL: shuffle_points off (explicit mode)
    uint64_t seed;
    int seeded, shuffle;
};

__global__ __launch_bounds__(256) void is_output_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off,
                                                        int64_t n_total, int c, int64_t n_cap, int k, Draws d,
                                                        int32_t* __restrict__ info, const int32_t* __restrict__ mlist,
                                                        const int32_t* __restrict__ plist, float* __restrict__ out) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= k) return;
    const int n = info[b * 4 + 0], n_far = info[b * 4 + 1];
    const int bad = info[b * 4 + 3] & (ST_BAD_OFFSETS | ST_OVER_CAP);
    const int64_t row = (int64_t)b * k;
    const int64_t base = (int64_t)b * n_cap;
    int src = -1;
    if (n > 0 && !bad) {
        int t = j;
        if (d.shuffle) t = d.seeded ? (int)keyed_bijection(stream_key(d.seed, b, 2), (uint32_t)k, (uint32_t)j) : d.perm2[row + j];
        int i = -1;
        if (t >= 0 && t < k) i = d.seeded ? (int)keyed_bijection(stream_key(d.seed, b, 1), (uint32_t)k, (uint32_t)t) : d.perm1[row + t];
        if (i >= 0 && i < k) {
            const uint64_t kp = stream_key(d.seed, b, 0);
            if (n > k) {
                const int n_near = n - n_far;
                if (n_far < k) {                                   // (A)
                    const int r = k - n_far;
                    if (i < r) {
                        const int q = d.seeded ? (int)keyed_bijection(kp, (uint32_t)n_near, (uint32_t)i) : d.pick[row + i];
                        if (q >= 0 && q < n_near) src = plist[base + q];
                    } else {
                        src = plist[base + n_near + (i - r)];
                    }
                } else {                                           // (B)
                    const int q = d.seeded ? (int)keyed_bijection(kp, (uint32_t)n, (uint32_t)i) : d.pick[row + i];
                    if (q >= 0 && q < n) src = mlist[base + q];
                }
            } else if (i < n) {                                    // (C)
                src = mlist[base + i];
            } else {
                const int q = d.seeded ? (int)draw_below(kp, (uint32_t)(i - n), (uint32_t)n) : d.pick[row + (i - n)];
                if (q >= 0 && q < n) src = mlist[base + q];
            }
        }
        if (src < 0) atomicOr(info + b * 4 + 3, ST_BAD_DRAW);
    }
    float* o = out + (row + j) * (int64_t)(1 + c);
    o[0] = (float)b;
    if (src >= 0) {
        const float* p = pts + (off[b] + src) * (int64_t)c;
        for (int f = 0; f < c; ++f) o[1 + f] = p[f];
    } else {
        for (int f = 0; f < c; ++f) o[1 + f] = 0.f;
    }
}

// One workgroup per scene: REMOVE_OUTSIDE_BOXES (box_utils.mask_boxes_outside_range_numpy) + collate_batch's zero padding.
// Corners: the template (+-dx/2, +-dy/2, +-dz/2) of boxes_to_corners_3d rotated about z as
// common_utils.rotate_points_along_z does ([x, y] times [[cos, sin], [-sin, cos]]), then shifted to the centre.
__global__ __launch_bounds__(256) void is_boxes_kernel(const float* __restrict__ boxes, const int64_t* __restrict__ boff,
                                                       int64_t m_total, int dim, int max_gt, Range rg, int min_corners,
                                                       float* __restrict__ gt, int32_t* __restrict__ info) {
    __shared__ int32_t wk[4];
    __shared__ int32_t kept_sh;
    const int b = blockIdx.x;
    const int64_t s = boff[b], e = boff[b + 1];
    const bool ok = s >= 0 && e >= s && e <= m_total && e - s <= INT32_MAX;
    const int m = ok ? (int)(e - s) : 0;
    if (threadIdx.x == 0) kept_sh = 0;
    __syncthreads();
    float* g = gt + (int64_t)b * max_gt * dim;
    for (int c0 = 0; c0 < m; c0 += 256) {
        const int i = c0 + (int)threadIdx.x;
        bool keep = false;
        if (i < m) {
            const float* p = boxes + (s + i) * (int64_t)dim;
            const float cx = p[0], cy = p[1], cz = p[2], hx = p[3] * 0.5f, hy = p[4] * 0.5f, hz = p[5] * 0.5f;
            const float ca = cosf(p[6]), sa = sinf(p[6]);
            int inside = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float lx = (q == 0 || q == 1 || q == 4 || q == 5) ? hx : -hx;
                const float ly = (q == 0 || q == 3 || q == 4 || q == 7) ? hy : -hy;
                const float lz = q < 4 ? -hz : hz;
                const float x = (lx * ca + ly * -sa) + cx, y = (lx * sa + ly * ca) + cy, z = lz + cz;
                inside += (x >= rg.lo[0] && x <= rg.hi[0] && y >= rg.lo[1] && y <= rg.hi[1] && z >= rg.lo[2] && z <= rg.hi[2]) ? 1 : 0;
            }
            keep = inside >= min_corners;
        }
        const uint64_t bk = __ballot(keep);
        const int w = wave_id();
        if (lane_id() == 0) wk[w] = __popcll(bk);
        __syncthreads();
        int pos = kept_sh + rank_below(bk);
        for (int v = 0; v < w; ++v) pos += wk[v];
        if (keep && pos < max_gt) {
            const float* p = boxes + (s + i) * (int64_t)dim;
            for (int f = 0; f < dim; ++f) g[(int64_t)pos * dim + f] = p[f];
        }
        __syncthreads();
        if (threadIdx.x == 0) kept_sh += wk[0] + wk[1] + wk[2] + wk[3];
        __syncthreads();
    }
    const int kept = kept_sh;
    for (int64_t x = (int64_t)min(kept, max_gt) * dim + threadIdx.x; x < (int64_t)max_gt * dim; x += 256) g[x] = 0.f;
    if (threadIdx.x == 0) info[b * 4 + 2] = ok ? kept : -1;
}

int64_t tiles_of(int64_t n_cap) { return divup64(n_cap, IS_TILE); }
int64_t tile_bytes(int batch, int64_t n_cap) { return (batch * tiles_of(n_cap) * 2 * 4 + 255) / 256 * 256; }

Range range_of(const float* r6) {
    Range rg;
    for (int a = 0; a < 3; ++a) { rg.lo[a] = r6[a]; rg.hi[a] = r6[3 + a]; }
    return rg;
}

}  // namespace
}  // namespace pda

PDA_API int64_t pda_input_stage_workspace_bytes(int batch, int64_t n_cap) {
    if (!pda::stage_sizes_ok(batch, n_cap)) return -1;
    return pda::tile_bytes(batch, n_cap) + 2 * (int64_t)batch * n_cap * 4;
}

PDA_API int pda_input_stage(const float* points, const int64_t* offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                            const float* range6, int num_points, const int32_t* pick, const int32_t* perm1, const int32_t* perm2,
                            uint64_t seed, int shuffle, float* out_points, int32_t* info, void* workspace, pda_stream_t stream) {
    PDA_REQUIRE(pda::stage_sizes_ok(batch, n_cap) && n_total >= 0 && c >= 3 && c <= 64 && num_points >= 1 &&
                    num_points <= (1 << 30) && (shuffle == 0 || shuffle == 1),
                "pda_input_stage: bad size: batch=%d n_total=%lld C=%d n_cap=%lld num_points=%d shuffle=%d", batch,
                (long long)n_total, c, (long long)n_cap, num_points, shuffle);
    if (batch == 0) return PDA_OK;
    // the mode follows from which draw pointers are NULL; checked before the required pointers
    const bool seeded = pick == nullptr;
    PDA_REQUIRE(seeded == (perm1 == nullptr), "pda_input_stage: pick and perm1 are both given (explicit mode) or both NULL (seeded)");
    PDA_REQUIRE(seeded || (perm2 != nullptr) == (shuffle == 1), "pda_input_stage: explicit mode: perm2 is given exactly when shuffle == 1");
    PDA_REQUIRE(!seeded || perm2 == nullptr, "pda_input_stage: seeded mode takes no perm2");
    PDA_REQUIRE(range6 && offsets && out_points && info && workspace && (points || n_total == 0), "pda_input_stage: null pointer");
    const pda::Range rg = pda::range_of(range6);
    const int tiles = (int)pda::tiles_of(n_cap);
    int32_t* tile_cnt = (int32_t*)workspace;
    int32_t* mlist = (int32_t*)((char*)workspace + pda::tile_bytes(batch, n_cap));
    int32_t* plist = mlist + (int64_t)batch * n_cap;
    hipStream_t st = (hipStream_t)stream;
    const dim3 tgrid((unsigned)tiles, (unsigned)batch);
    hipLaunchKernelGGL(pda::is_count_kernel, tgrid, dim3(pda::IS_TILE), 0, st, points, offsets, n_total, c, n_cap, rg, tiles, tile_cnt);
    hipLaunchKernelGGL(pda::is_scan_kernel, dim3((unsigned)batch), dim3(1024), 0, st, offsets, n_total, n_cap, tiles, tile_cnt, info);
    hipLaunchKernelGGL(pda::is_scatter_kernel, tgrid, dim3(pda::IS_TILE), 0, st, points, offsets, n_total, c, n_cap, rg, tiles,
                       tile_cnt, info, mlist, plist);
    const pda::Draws d{pick, perm1, perm2, seed, seeded ? 1 : 0, shuffle};
    hipLaunchKernelGGL(pda::is_output_kernel, dim3((unsigned)pda::divup(num_points, 256), (unsigned)batch), dim3(256), 0, st, points,
                       offsets, n_total, c, n_cap, num_points, d, info, mlist, plist, out_points);
    return pda::check_launch("pda_input_stage");
}

PDA_API int pda_input_boxes(const float* boxes, const int64_t* box_offsets, int64_t m_total, int batch, int box_dim, int max_gt,
                            const float* range6, int min_num_corners, float* gt_boxes, int32_t* info, pda_stream_t stream) {
    PDA_REQUIRE(batch >= 0 && batch <= (1 << 24) && m_total >= 0 && box_dim >= 7 && box_dim <= 64 && max_gt >= 0 &&
                    max_gt <= (1 << 20) && min_num_corners >= 0 && min_num_corners <= 8,
                "pda_input_boxes: bad size: batch=%d m_total=%lld box_dim=%d max_gt=%d min_num_corners=%d", batch,
                (long long)m_total, box_dim, max_gt, min_num_corners);
    if (batch == 0) return PDA_OK;
    PDA_REQUIRE(range6 && box_offsets && info && (boxes || m_total == 0) && (gt_boxes || max_gt == 0),
                "pda_input_boxes: null pointer");
    hipLaunchKernelGGL(pda::is_boxes_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, boxes, box_offsets, m_total,
                       box_dim, max_gt, pda::range_of(range6), min_num_corners, gt_boxes, info);
    return pda::check_launch("pda_input_boxes");
}
