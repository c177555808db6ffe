// voxel_stage.hip -- point-to-voxel on the device (include/pda_train.h, pda_voxelize / pda_voxel_sample): the reference's
// VoxelGeneratorWrapper.generate (spconv's CPU point-to-voxel loop) and DataProcessor.sample_points_by_voxels up to the point
// where sample_points takes over (pcdet/datasets/processor/data_processor.py).
//
// The loop to reproduce, per scene, over the points in their (optionally masked and shuffled) order:
//   c_j = floor((p_j - lo_j) / vs_j) in float32 (correctly rounded divide); a point with a c_j outside [0, grid_j) joins nothing;
//   a cell seen for the first time becomes voxel number voxel_num++ unless voxel_num >= max_voxels (then the point is skipped,
//   later points of existing voxels still join); a voxel keeps its first max_points points.
// Nothing here depends on the order threads run in:
//   * a hash table per scene (open addressing, power-of-two capacity >= 2 * n_cap) of 64-bit entries (cell key << 32 | position):
//     a slot is claimed by compare-and-swap and lowered with a 64-bit atomic min, so whichever slot a key lands in, the table
//     ends with the smallest position of every occupied cell; a key never leaves the slot it claimed, so a cell has one slot;
//   * a point is its voxel's first iff it holds that minimum; the stable ballot / mbcnt compaction of the first points numbers
//     the voxels in order of first appearance; "voxel number >= max_voxels" is the cap;
//   * the r-th point of a voxel (r = 1 .. max_points - 1) is the minimum over the points not yet placed: one 32-bit atomic min
//     per round into a second array, which the round's winner resets.
// Launches (all sized from batch, n_cap and max_voxels; no host read):
//   vx_mask_count / vx_mask_scan / vx_mask_scatter : mlist = the points inside the x / y limits (or all), in order;
//   vx_insert        : position s of the shuffled order -> raw row, cell, table slot;
//   vx_first_count / vx_first_scan / vx_offsets / vx_first_scatter : the first points, voxel numbers, rank-0 output;
//   vx_round_min / vx_round_settle (max_points - 1 times, not for SAMPLE_TYPE raw) : ranks 1 ..;
//   vx_mean          : SAMPLE_TYPE mean_vfe, one thread per voxel.
// Integer atomics only; the file is built with -ffp-contract=off.
#include "pda_common.h"
#include "ragged_scene.h"
#include "stage_rng.h"
#include "voxel_cell.h"

namespace pda {
namespace {

constexpr int VX_TILE = 256;
constexpr int VX_WAVES = VX_TILE / PDA_WAVE;
// info[b][3] status bits of this stage (include/pda_train.h), next to ragged_scene.h's
constexpr int ST_EMPTY = 1, ST_BAD_DRAW = 8, ST_VOXEL_CAP = 16;
constexpr int ST_UNUSABLE = ST_BAD_OFFSETS | ST_OVER_CAP | ST_BAD_DRAW;
constexpr uint64_t VX_EMPTY = ~0ull;
constexpr uint32_t VX_NONE = 0xffffffffu;
constexpr int MODE_RAW = 0, MODE_MEAN = 1, MODE_VOXELS = 2;

struct Grid {
    float lo[3], vs[3];
    float xy[4];       // xmin, ymin, xmax, ymax of the range mask
    int32_t n[3];      // cells along x, y, z
    int mask;          // 1: the x / y range mask of mask_points_and_boxes_outside_range comes first
};

__device__ __forceinline__ uint64_t perm0_key(uint64_t seed, int b) {
    return splitmix64(~seed ^ splitmix64(0x766f78656c5f7030ull + (uint64_t)b));
}

// The cell of a point (voxel_cell.h): false when a coordinate is NaN or falls outside the grid.
__device__ __forceinline__ bool cell_of(const float* __restrict__ p, const Grid& g, uint32_t& key) {
    uint32_t c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (!cell_axis(p[a], g.lo[a], g.vs[a], g.n[a], c[a])) return false;
    key = (c[2] * (uint32_t)g.n[1] + c[1]) * (uint32_t)g.n[0] + c[0];
    return true;
}

__device__ __forceinline__ uint64_t load_relaxed(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t load_relaxed(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Exclusive scan of a scene's `tiles` pairs of tile counts in place by one workgroup of 1024 threads; thread u owns the `per`
// consecutive tiles from u * per.  The totals are valid in every thread.
__device__ __forceinline__ void scan_tiles(int32_t* __restrict__ tc, int tiles, int32_t& tot0, int32_t& tot1) {
    __shared__ int32_t p0[1024], p1[1024];
    const int u = threadIdx.x;
    const int per = (tiles + 1023) / 1024;
    const int t0 = min(tiles, u * per), t1 = min(tiles, t0 + per);
    int32_t s0 = 0, s1 = 0;
    for (int t = t0; t < t1; ++t) { s0 += tc[2 * t]; s1 += tc[2 * t + 1]; }
    p0[u] = s0;
    p1[u] = s1;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {          // Hillis-Steele inclusive scan of the 1024 partial sums
        const int32_t v0 = u >= o ? p0[u - o] : 0, v1 = u >= o ? p1[u - o] : 0;
        __syncthreads();
        p0[u] += v0;
        p1[u] += v1;
        __syncthreads();
    }
    int32_t r0 = p0[u] - s0, r1 = p1[u] - s1;
    for (int t = t0; t < t1; ++t) {
        const int32_t c0 = tc[2 * t], c1 = tc[2 * t + 1];
        tc[2 * t] = r0;
        tc[2 * t + 1] = r1;
        r0 += c0;
        r1 += c1;
    }
    tot0 = p0[1023];
    tot1 = p1[1023];
}

// Sums a flag pair over the workgroup's tile and stores it as the tile's counts.
__device__ __forceinline__ void store_tile_counts(bool f0, bool f1, int32_t* __restrict__ o) {
    __shared__ int32_t w0[VX_WAVES], w1[VX_WAVES];
    const uint64_t b0 = __ballot(f0), b1 = __ballot(f1);
    if (lane_id() == 0) {
        w0[wave_id()] = __popcll(b0);
        w1[wave_id()] = __popcll(b1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t s0 = 0, s1 = 0;
        for (int w = 0; w < VX_WAVES; ++w) { s0 += w0[w]; s1 += w1[w]; }
        o[0] = s0;
        o[1] = s1;
    }
}

// Position of a flagged thread among the flagged threads of its tile (every thread of the workgroup calls this).
__device__ __forceinline__ int tile_rank(bool f) {
    __shared__ int32_t wc[VX_WAVES];
    const uint64_t bal = __ballot(f);
    const int w = wave_id();
    if (lane_id() == 0) wc[w] = __popcll(bal);
    __syncthreads();
    int pos = rank_below(bal);
    for (int v = 0; v < w; ++v) pos += wc[v];
    return pos;
}

__device__ __forceinline__ bool in_mask(const float* __restrict__ pts, const Scene& s, int i, int c, const Grid& g) {
    if (i >= s.n) return false;
    if (!g.mask) return true;
    const float* p = pts + (s.start + i) * (int64_t)c;
    const float x = p[0], y = p[1];
    if (is_nan_bits(x) || is_nan_bits(y)) return false;
    return x >= g.xy[0] && x <= g.xy[2] && y >= g.xy[1] && y <= g.xy[3];
}

// ---- the range mask ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VX_TILE) void vx_mask_count(const float* __restrict__ pts, const int64_t* __restrict__ off,
                                                         int64_t n_total, int c, int64_t n_cap, Grid g, int tiles,
                                                         int32_t* __restrict__ tile_cnt) {
    const int b = blockIdx.y, t = blockIdx.x;
    const Scene s = scene_of(off, b, n_total, n_cap);
    const bool m = in_mask(pts, s, t * VX_TILE + (int)threadIdx.x, c, g);
    store_tile_counts(m, false, tile_cnt + ((int64_t)b * tiles + t) * 2);
}

// One workgroup per scene.  info = [n_masked, 0, 0, status]; an explicit perm0 slice of another length than n_masked is a
// bad draw.
__global__ __launch_bounds__(1024) void vx_mask_scan(const int64_t* __restrict__ off, int64_t n_total, int64_t n_cap, int tiles,
                                                     const int64_t* __restrict__ poff, int64_t perm0_total,
                                                     int32_t* __restrict__ tile_cnt, int32_t* __restrict__ info) {
    const int b = blockIdx.x;
    int32_t n, unused;
    scan_tiles(tile_cnt + (int64_t)b * tiles * 2, tiles, n, unused);
    if (threadIdx.x == 0) {
        int status = scene_of(off, b, n_total, n_cap).status;
        if (poff) {
            const int64_t ps = poff[b], pe = poff[b + 1];
            if (ps < 0 || pe < ps || pe > perm0_total || pe - ps != (int64_t)n) status |= ST_BAD_DRAW;
        }
        info[b * 4 + 0] = n;
        info[b * 4 + 1] = 0;
        info[b * 4 + 2] = 0;
        info[b * 4 + 3] = status;
    }
}

__global__ __launch_bounds__(VX_TILE) void vx_mask_scatter(const float* __restrict__ pts, const int64_t* __restrict__ off,
                                                           int64_t n_total, int c, int64_t n_cap, Grid g, int tiles,
                                                           const int32_t* __restrict__ tile_off, int32_t* __restrict__ mlist) {
    const int b = blockIdx.y, t = blockIdx.x;
    const Scene s = scene_of(off, b, n_total, n_cap);
    const int i = t * VX_TILE + (int)threadIdx.x;
    const bool m = in_mask(pts, s, i, c, g);
    const int pos = tile_off[((int64_t)b * tiles + t) * 2] + tile_rank(m);
    if (m) mlist[(int64_t)b * n_cap + pos] = i;          // pos < n_masked <= n_cap
}

// ---- the table ---------------------------------------------------------------------------------------------------------
struct Shuffle {
    const int32_t* perm0;    // explicit mode: ragged, scene b at poff[b]; NULL: seeded (when on) or no shuffle
    const int64_t* poff;
    uint64_t seed;
    int on;
};

// Thread s = a position of the scene's shuffled order.  src[s] = its raw row, slot[s] = the table slot of its cell (-1: it
// joins nothing).
__global__ __launch_bounds__(VX_TILE) void vx_insert(const float* __restrict__ pts, const int64_t* __restrict__ off, int c,
                                                     int64_t n_cap, Grid g, Shuffle sh, uint32_t cap_mask,
                                                     const int32_t* __restrict__ mlist, int32_t* __restrict__ info,
                                                     uint64_t* __restrict__ table, int32_t* __restrict__ src,
                                                     int32_t* __restrict__ slot) {
    const int b = blockIdx.y, s = blockIdx.x * VX_TILE + (int)threadIdx.x;
    const int n = info[b * 4 + 0];
    if (s >= n || (info[b * 4 + 3] & ST_UNUSABLE)) return;
    const int64_t base = (int64_t)b * n_cap;
    int q = s;
    if (sh.on) q = sh.perm0 ? sh.perm0[sh.poff[b] + s] : (int)keyed_bijection(perm0_key(sh.seed, b), (uint32_t)n, (uint32_t)s);
    int raw = -1, sl = -1;
    if (q < 0 || q >= n) {
        atomicOr(info + b * 4 + 3, ST_BAD_DRAW);
    } else {
        raw = mlist[base + q];
        uint32_t key;
        if (cell_of(pts + (off[b] + raw) * (int64_t)c, g, key)) {
            uint64_t* tab = table + (int64_t)b * ((int64_t)cap_mask + 1);
            const uint64_t e = ((uint64_t)key << 32) | (uint32_t)s;
            uint32_t h = mix32(key) & cap_mask;
            // at most n_cap <= capacity / 2 keys: an empty slot is always met; the bound only keeps a broken table from spinning
            for (uint32_t probes = 0; probes <= cap_mask; ++probes) {
                uint64_t cur = load_relaxed(tab + h);
                if (cur == VX_EMPTY) {
                    cur = atomicCAS((unsigned long long*)(tab + h), (unsigned long long)VX_EMPTY, (unsigned long long)e);
                    if (cur == VX_EMPTY) { sl = (int)h; break; }
                }
                if ((uint32_t)(cur >> 32) == key) {
                    atomicMin((unsigned long long*)(tab + h), (unsigned long long)e);
                    sl = (int)h;
                    break;
                }
                h = (h + 1) & cap_mask;
            }
        }
    }
    src[base + s] = raw;
    slot[base + s] = sl;
}

__device__ __forceinline__ void first_flags(int b, int s, int64_t n_cap, uint32_t cap_mask, const int32_t* __restrict__ info,
                                            const uint64_t* __restrict__ table, const int32_t* __restrict__ slot,
                                            bool& in_grid, bool& first) {
    in_grid = first = false;
    if (s >= info[b * 4 + 0] || (info[b * 4 + 3] & ST_UNUSABLE)) return;
    const int sl = slot[(int64_t)b * n_cap + s];
    if (sl < 0) return;
    in_grid = true;
    first = (uint32_t)table[(int64_t)b * ((int64_t)cap_mask + 1) + sl] == (uint32_t)s;
}

__global__ __launch_bounds__(VX_TILE) void vx_first_count(int64_t n_cap, uint32_t cap_mask, int tiles,
                                                          const int32_t* __restrict__ info, const uint64_t* __restrict__ table,
                                                          const int32_t* __restrict__ slot, int32_t* __restrict__ tile_cnt) {
    const int b = blockIdx.y, t = blockIdx.x;
    bool in_grid, first;
    first_flags(b, t * VX_TILE + (int)threadIdx.x, n_cap, cap_mask, info, table, slot, in_grid, first);
    store_tile_counts(first, in_grid, tile_cnt + ((int64_t)b * tiles + t) * 2);
}

__global__ __launch_bounds__(1024) void vx_first_scan(int tiles, int max_voxels, int32_t* __restrict__ tile_cnt,
                                                      int32_t* __restrict__ info) {
    const int b = blockIdx.x;
    int32_t n_vox, n_in;
    scan_tiles(tile_cnt + (int64_t)b * tiles * 2, tiles, n_vox, n_in);
    if (threadIdx.x == 0) {
        info[b * 4 + 1] = n_in;
        info[b * 4 + 2] = n_vox;
        info[b * 4 + 3] |= (n_vox == 0 ? ST_EMPTY : 0) | (n_vox > max_voxels ? ST_VOXEL_CAP : 0);
    }
}

// One workgroup: out_offsets = the exclusive scan of the scenes' kept voxel counts (batch + 1 entries); num_voxels (batch),
// when given, = the kept count, -1 for a scene whose offsets are unusable.
__global__ __launch_bounds__(1024) void vx_offsets(int batch, int max_voxels, const int32_t* __restrict__ info,
                                                   int64_t* __restrict__ out_offsets, int32_t* __restrict__ num_voxels) {
    __shared__ int64_t part[1024];
    const int u = threadIdx.x;
    const int per = (batch + 1023) / 1024;
    const int b0 = min(batch, u * per), b1 = min(batch, b0 + per);
    int64_t sum = 0;
    for (int b = b0; b < b1; ++b) sum += min(info[b * 4 + 2], max_voxels);
    part[u] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t v = u >= o ? part[u - o] : 0;
        __syncthreads();
        part[u] += v;
        __syncthreads();
    }
    int64_t run = part[u] - sum;
    for (int b = b0; b < b1; ++b) {
        const int kept = min(info[b * 4 + 2], max_voxels);
        if (out_offsets) out_offsets[b] = run;
        if (num_voxels) num_voxels[b] = (info[b * 4 + 3] & (ST_BAD_OFFSETS | ST_OVER_CAP)) ? -1 : kept;
        run += kept;
    }
    if (u == 1023 && out_offsets) out_offsets[batch] = part[1023];
}

struct Out {
    int mode;                  // MODE_RAW / MODE_MEAN / MODE_VOXELS
    int max_voxels, max_points;
    int64_t vcap;              // min(n_cap, max_voxels): rows of member / npv a scene owns (MODE_MEAN)
    float* out_points;         // MODE_RAW, MODE_MEAN: packed rows, scene b from out_offsets[b]
    const int64_t* out_offsets;
    int32_t* member;           // MODE_MEAN: (batch, vcap, max_points) raw rows of a voxel's points
    int32_t* npv;              // MODE_MEAN: (batch, vcap); MODE_VOXELS: (batch, max_voxels) points a voxel holds
    float* voxels;             // MODE_VOXELS: (batch, max_voxels, max_points, C)
    int32_t* coords;           // MODE_VOXELS: (batch, max_voxels, 3) z, y, x
};

// Point `raw` of scene b becomes point number r of voxel v (v < max_voxels, r < max_points).
__device__ __forceinline__ void place(const Out& o, const float* __restrict__ p, int c, int b, int v, int r, int raw) {
    if (o.mode == MODE_MEAN) {
        const int64_t at = (int64_t)b * o.vcap + v;
        o.member[at * o.max_points + r] = raw;
        o.npv[at] = r + 1;
    } else if (o.mode == MODE_VOXELS) {
        const int64_t at = (int64_t)b * o.max_voxels + v;
        float* d = o.voxels + (at * o.max_points + r) * (int64_t)c;
        for (int f = 0; f < c; ++f) d[f] = p[f];
        o.npv[at] = r + 1;
    }
}

// The first points in their order = the voxels in order of first appearance: voxnum[first position] = the voxel's number, and
// its point number 0.
__global__ __launch_bounds__(VX_TILE) void vx_first_scatter(const float* __restrict__ pts, const int64_t* __restrict__ off, int c,
                                                            int64_t n_cap, Grid g, uint32_t cap_mask, int tiles,
                                                            const int32_t* __restrict__ tile_off, const int32_t* __restrict__ info,
                                                            const uint64_t* __restrict__ table, const int32_t* __restrict__ src,
                                                            int32_t* __restrict__ slot, int32_t* __restrict__ voxnum, Out o) {
    const int b = blockIdx.y, t = blockIdx.x, s = t * VX_TILE + (int)threadIdx.x;
    bool in_grid, first;
    first_flags(b, s, n_cap, cap_mask, info, table, slot, in_grid, first);
    const int v = tile_off[((int64_t)b * tiles + t) * 2] + tile_rank(first);
    if (!first) return;
    const int64_t base = (int64_t)b * n_cap;
    const int sl = slot[base + s];
    voxnum[base + s] = v;
    slot[base + s] = -1;                                  // placed (or refused): takes no part in the rounds
    if (v >= o.max_voxels) return;
    const int raw = src[base + s];
    const float* p = pts + (off[b] + raw) * (int64_t)c;
    if (o.mode == MODE_RAW) {
        float* d = o.out_points + (o.out_offsets[b] + v) * (int64_t)c;
        for (int f = 0; f < c; ++f) d[f] = p[f];
        return;
    }
    place(o, p, c, b, v, 0, raw);
    if (o.mode == MODE_VOXELS) {
        uint32_t key = (uint32_t)(table[(int64_t)b * ((int64_t)cap_mask + 1) + sl] >> 32);
        int32_t* cd = o.coords + ((int64_t)b * o.max_voxels + v) * 3;
        cd[2] = (int32_t)(key % (uint32_t)g.n[0]);
        key /= (uint32_t)g.n[0];
        cd[1] = (int32_t)(key % (uint32_t)g.n[1]);
        cd[0] = (int32_t)(key / (uint32_t)g.n[1]);
    }
}

// ---- points 1 .. max_points - 1 of every voxel ---------------------------------------------------------------------------
// Round r: every point not yet placed lowers cur[slot] to its position ...
__global__ __launch_bounds__(VX_TILE) void vx_round_min(int64_t n_cap, uint32_t cap_mask, int max_voxels, int round,
                                                        const int32_t* __restrict__ info, const uint64_t* __restrict__ table,
                                                        const int32_t* __restrict__ voxnum, int32_t* __restrict__ slot,
                                                        uint32_t* __restrict__ cur) {
    const int b = blockIdx.y, s = blockIdx.x * VX_TILE + (int)threadIdx.x;
    if (s >= info[b * 4 + 0] || (info[b * 4 + 3] & ST_UNUSABLE)) return;
    const int64_t base = (int64_t)b * n_cap, tbase = (int64_t)b * ((int64_t)cap_mask + 1);
    const int sl = slot[base + s];
    if (sl < 0) return;
    if (round == 1 && voxnum[base + (uint32_t)table[tbase + sl]] >= max_voxels) {      // a voxel the cap refused
        slot[base + s] = -1;
        return;
    }
    atomicMin(cur + tbase + sl, (uint32_t)s);
}

// ... and the point that holds the minimum becomes the voxel's point number r and frees cur[slot] for the next round.  The
// other points of the cell read cur[slot] while the winner resets it: they see the winner's position or VX_NONE, never
// their own.
__global__ __launch_bounds__(VX_TILE) void vx_round_settle(const float* __restrict__ pts, const int64_t* __restrict__ off, int c,
                                                           int64_t n_cap, uint32_t cap_mask, int round,
                                                           const int32_t* __restrict__ info, const uint64_t* __restrict__ table,
                                                           const int32_t* __restrict__ src, const int32_t* __restrict__ voxnum,
                                                           int32_t* __restrict__ slot, uint32_t* __restrict__ cur, Out o) {
    const int b = blockIdx.y, s = blockIdx.x * VX_TILE + (int)threadIdx.x;
    if (s >= info[b * 4 + 0] || (info[b * 4 + 3] & ST_UNUSABLE)) return;
    const int64_t base = (int64_t)b * n_cap, tbase = (int64_t)b * ((int64_t)cap_mask + 1);
    const int sl = slot[base + s];
    if (sl < 0 || load_relaxed(cur + tbase + sl) != (uint32_t)s) return;
    const int v = voxnum[base + (uint32_t)table[tbase + sl]];
    const int raw = src[base + s];
    place(o, pts + (off[b] + raw) * (int64_t)c, c, b, v, round, raw);
    slot[base + s] = -1;
    __hip_atomic_store(cur + tbase + sl, VX_NONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// SAMPLE_TYPE mean_vfe: numpy's voxels.sum(axis=1) / num_points -- the float32 sum over all max_points slots in slot order
// (the zero padding included: -0 + 0 = +0), then the division in float64, rounded to float32.
__global__ __launch_bounds__(256) void vx_mean(const float* __restrict__ pts, const int64_t* __restrict__ off, int c,
                                               const int32_t* __restrict__ info, Out o) {
    const int b = blockIdx.y, v = blockIdx.x * 256 + (int)threadIdx.x;
    if ((info[b * 4 + 3] & ST_UNUSABLE) || v >= min(info[b * 4 + 2], o.max_voxels)) return;
    const int64_t at = (int64_t)b * o.vcap + v;
    const int cnt = o.npv[at];
    const int32_t* mem = o.member + at * o.max_points;
    float* d = o.out_points + (o.out_offsets[b] + v) * (int64_t)c;
    const float* rows = pts + off[b] * (int64_t)c;
    for (int f = 0; f < c; ++f) {
        float acc = rows[(int64_t)mem[0] * c + f];
        for (int r = 1; r < o.max_points; ++r) {
            const float x = rows[(int64_t)mem[r < cnt ? r : 0] * c + f];      // slots beyond cnt were never written
            acc = acc + (r < cnt ? x : 0.f);
        }
        d[f] = (float)((double)acc / (double)cnt);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
constexpr uint64_t VX_MAX_CELLS = 0xffffffffull;      // keys are 32 bits and 0xffffffff marks an empty slot
constexpr int VX_MAX_DIM = 1 << 24;                   // (float)cells along an axis is exact

int64_t tiles_of(int64_t n_cap) { return divup64(n_cap, VX_TILE); }
int64_t pad256(int64_t x) { return (x + 255) / 256 * 256; }
int64_t capacity_of(int64_t n_cap) {
    int64_t cap = 2;
    while (cap < 2 * n_cap) cap <<= 1;
    return cap;
}
bool sizes_ok(int batch, int64_t n_cap, int max_voxels, int max_points) {
    return batch >= 0 && batch <= 65535 && n_cap >= 1 && n_cap <= (1 << 30) && max_voxels >= 1 && max_voxels <= (1 << 30) &&
           max_points >= 1 && max_points <= 64;
}

struct Layout {
    int64_t table, cur, info, tile_cnt, mlist, src, slot, voxnum, member, npv, total;
};
Layout layout_of(int batch, int64_t n_cap, int max_voxels, int max_points) {
    const int64_t cap = capacity_of(n_cap), vcap = n_cap < max_voxels ? n_cap : max_voxels, list = pad256(batch * n_cap * 4);
    Layout l;
    int64_t at = 0;
    l.table = at; at += pad256(batch * cap * 8);
    l.cur = at; at += pad256(batch * cap * 4);
    l.info = at; at += pad256((int64_t)batch * 16);
    l.tile_cnt = at; at += pad256(batch * tiles_of(n_cap) * 2 * 4);
    l.mlist = at; at += list;
    l.src = at; at += list;
    l.slot = at; at += list;
    l.voxnum = at; at += list;
    l.member = at; at += pad256(batch * vcap * max_points * 4);
    l.npv = at; at += pad256(batch * vcap * 4);
    l.total = at;
    return l;
}

// Host-side checks of the grid: false with the error set.
bool grid_of(const char* who, const float* range6, const float* vs3, const int32_t* grid3, int mask, Grid& g) {
    uint64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = range6[a];
        g.vs[a] = vs3[a];
        g.n[a] = grid3[a];
        if (!(vs3[a] > 0.f) || !(vs3[a] < 3.0e38f) || grid3[a] < 1 || grid3[a] > VX_MAX_DIM) {
            set_error("%s: bad grid: voxel size %g, %d cells along axis %d (1 .. %d cells an axis)", who, (double)vs3[a], grid3[a], a,
                      VX_MAX_DIM);
            return false;
        }
        cells *= (uint64_t)grid3[a];
        if (cells > VX_MAX_CELLS) {
            set_error("%s: grid %d x %d x %d holds more than %llu cells, the most a 32-bit cell key holds", who, grid3[0], grid3[1],
                      grid3[2], (unsigned long long)VX_MAX_CELLS);
            return false;
        }
    }
    g.xy[0] = range6[0]; g.xy[1] = range6[1]; g.xy[2] = range6[3]; g.xy[3] = range6[4];
    g.mask = mask;
    return true;
}

// Everything both entries share.  The outputs of `o` are set by the caller; member / npv (MODE_MEAN) come from the workspace.
int run(const char* who, const float* points, const int64_t* offsets, int64_t n_total, int batch, int c, int64_t n_cap,
        const Grid& g, Shuffle sh, int64_t perm0_total, Out o, int64_t* out_offsets, int32_t* num_voxels, int32_t* info,
        void* workspace, hipStream_t st) {
    const Layout l = layout_of(batch, n_cap, o.max_voxels, o.max_points);
    char* ws = (char*)workspace;
    uint64_t* table = (uint64_t*)(ws + l.table);
    uint32_t* cur = (uint32_t*)(ws + l.cur);
    if (!info) info = (int32_t*)(ws + l.info);
    int32_t* tile_cnt = (int32_t*)(ws + l.tile_cnt);
    int32_t* mlist = (int32_t*)(ws + l.mlist);
    int32_t* src = (int32_t*)(ws + l.src);
    int32_t* slot = (int32_t*)(ws + l.slot);
    int32_t* voxnum = (int32_t*)(ws + l.voxnum);
    if (o.mode == MODE_MEAN) {
        o.member = (int32_t*)(ws + l.member);
        o.npv = (int32_t*)(ws + l.npv);
    }
    const int tiles = (int)tiles_of(n_cap);
    const uint32_t cap_mask = (uint32_t)(capacity_of(n_cap) - 1);
    const int rounds = o.mode == MODE_RAW ? 1 : o.max_points;
    // table and cur are adjacent: one fill with 0xff empties both
    if (hipMemsetAsync(table, 0xff, (size_t)(rounds > 1 ? l.info - l.table : l.cur - l.table), st) != hipSuccess)
        return check_launch(who);
    const dim3 tgrid((unsigned)tiles, (unsigned)batch), tblock(VX_TILE);
    hipLaunchKernelGGL(vx_mask_count, tgrid, tblock, 0, st, points, offsets, n_total, c, n_cap, g, tiles, tile_cnt);
    hipLaunchKernelGGL(vx_mask_scan, dim3((unsigned)batch), dim3(1024), 0, st, offsets, n_total, n_cap, tiles, sh.poff, perm0_total,
                       tile_cnt, info);
    hipLaunchKernelGGL(vx_mask_scatter, tgrid, tblock, 0, st, points, offsets, n_total, c, n_cap, g, tiles, tile_cnt, mlist);
    hipLaunchKernelGGL(vx_insert, tgrid, tblock, 0, st, points, offsets, c, n_cap, g, sh, cap_mask, mlist, info, table, src, slot);
    hipLaunchKernelGGL(vx_first_count, tgrid, tblock, 0, st, n_cap, cap_mask, tiles, info, table, slot, tile_cnt);
    hipLaunchKernelGGL(vx_first_scan, dim3((unsigned)batch), dim3(1024), 0, st, tiles, o.max_voxels, tile_cnt, info);
    hipLaunchKernelGGL(vx_offsets, dim3(1), dim3(1024), 0, st, batch, o.max_voxels, info, out_offsets, num_voxels);
    o.out_offsets = out_offsets;
    hipLaunchKernelGGL(vx_first_scatter, tgrid, tblock, 0, st, points, offsets, c, n_cap, g, cap_mask, tiles, tile_cnt, info, table,
                       src, slot, voxnum, o);
    for (int r = 1; r < rounds; ++r) {
        hipLaunchKernelGGL(vx_round_min, tgrid, tblock, 0, st, n_cap, cap_mask, o.max_voxels, r, info, table, voxnum, slot, cur);
        hipLaunchKernelGGL(vx_round_settle, tgrid, tblock, 0, st, points, offsets, c, n_cap, cap_mask, r, info, table, src, voxnum,
                           slot, cur, o);
    }
    if (o.mode == MODE_MEAN)
        hipLaunchKernelGGL(vx_mean, dim3((unsigned)divup64(o.vcap, 256), (unsigned)batch), dim3(256), 0, st, points, offsets, c, info,
                           o);
    return check_launch(who);
}

}  // namespace
}  // namespace pda

PDA_API int64_t pda_voxel_workspace_bytes(int batch, int64_t n_cap, int max_voxels, int max_points) {
    if (!pda::sizes_ok(batch, n_cap, max_voxels, max_points)) return -1;
    return pda::layout_of(batch, n_cap, max_voxels, max_points).total;
}

PDA_API int pda_voxel_sample(const float* points, const int64_t* offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                             const float* range6, const float* voxel_size3, const int32_t* grid3, int mask_xy, int max_voxels,
                             int max_points, int mean_vfe, int shuffle, const int32_t* perm0, const int64_t* perm0_offsets,
                             int64_t perm0_total, uint64_t seed, float* out_points, int64_t out_cap, int64_t* out_offsets,
                             int32_t* info, void* workspace, pda_stream_t stream) {
    PDA_REQUIRE(pda::sizes_ok(batch, n_cap, max_voxels, max_points) && n_total >= 0 && c >= 3 && c <= 64 &&
                    (mask_xy == 0 || mask_xy == 1) && (mean_vfe == 0 || mean_vfe == 1) && (shuffle == 0 || shuffle == 1) &&
                    perm0_total >= 0 && out_cap >= 0,
                "pda_voxel_sample: bad size: batch=%d n_total=%lld C=%d n_cap=%lld max_voxels=%d max_points=%d mask_xy=%d "
                "mean_vfe=%d shuffle=%d perm0_total=%lld out_cap=%lld",
                batch, (long long)n_total, c, (long long)n_cap, max_voxels, max_points, mask_xy, mean_vfe, shuffle,
                (long long)perm0_total, (long long)out_cap);
    PDA_REQUIRE(range6 && voxel_size3 && grid3, "pda_voxel_sample: null pointer (range6 / voxel_size3 / grid3)");
    pda::Grid g;
    if (!pda::grid_of("pda_voxel_sample", range6, voxel_size3, grid3, mask_xy, g)) return PDA_ERR_INVALID_ARGUMENT;
    if (batch == 0) return PDA_OK;
    PDA_REQUIRE((perm0 != nullptr) == (perm0_offsets != nullptr) && (perm0 == nullptr || shuffle == 1),
                "pda_voxel_sample: perm0 and perm0_offsets are given together, and only with shuffle == 1");
    const int64_t vcap = n_cap < max_voxels ? n_cap : max_voxels;
    PDA_REQUIRE(out_cap >= batch * vcap, "pda_voxel_sample: out_cap %lld is below batch * min(n_cap, max_voxels) = %lld",
                (long long)out_cap, (long long)(batch * vcap));
    PDA_REQUIRE(offsets && out_points && out_offsets && info && workspace && (points || n_total == 0),
                "pda_voxel_sample: null pointer");
    pda::Out o{};
    o.mode = mean_vfe ? pda::MODE_MEAN : pda::MODE_RAW;
    o.max_voxels = max_voxels;
    o.max_points = max_points;
    o.vcap = vcap;
    o.out_points = out_points;
    const pda::Shuffle sh{perm0, perm0_offsets, seed, shuffle};
    return pda::run("pda_voxel_sample", points, offsets, n_total, batch, c, n_cap, g, sh, perm0_total, o, out_offsets, nullptr, info,
                    workspace, (hipStream_t)stream);
}

PDA_API int pda_voxelize(const float* points, const int64_t* offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                         const float* range6, const float* voxel_size3, const int32_t* grid3, int max_voxels, int max_points,
                         float* voxels, int32_t* coords, int32_t* num_points_per_voxel, int32_t* num_voxels, void* workspace,
                         pda_stream_t stream) {
    PDA_REQUIRE(pda::sizes_ok(batch, n_cap, max_voxels, max_points) && n_total >= 0 && c >= 3 && c <= 64,
                "pda_voxelize: bad size: batch=%d n_total=%lld C=%d n_cap=%lld max_voxels=%d max_points=%d", batch,
                (long long)n_total, c, (long long)n_cap, max_voxels, max_points);
    PDA_REQUIRE(range6 && voxel_size3 && grid3, "pda_voxelize: null pointer (range6 / voxel_size3 / grid3)");
    pda::Grid g;
    if (!pda::grid_of("pda_voxelize", range6, voxel_size3, grid3, 0, g)) return PDA_ERR_INVALID_ARGUMENT;
    if (batch == 0) return PDA_OK;
    PDA_REQUIRE(offsets && voxels && coords && num_points_per_voxel && num_voxels && workspace && (points || n_total == 0),
                "pda_voxelize: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nv = (int64_t)batch * max_voxels;
    if (hipMemsetAsync(voxels, 0, (size_t)(nv * max_points * c * 4), st) != hipSuccess ||
        hipMemsetAsync(coords, 0, (size_t)(nv * 3 * 4), st) != hipSuccess ||
        hipMemsetAsync(num_points_per_voxel, 0, (size_t)(nv * 4), st) != hipSuccess)
        return pda::check_launch("pda_voxelize");
    pda::Out o{};
    o.mode = pda::MODE_VOXELS;
    o.max_voxels = max_voxels;
    o.max_points = max_points;
    o.vcap = n_cap < max_voxels ? n_cap : max_voxels;
    o.npv = num_points_per_voxel;
    o.voxels = voxels;
    o.coords = coords;
    const pda::Shuffle sh{nullptr, nullptr, 0, 0};
    return pda::run("pda_voxelize", points, offsets, n_total, batch, c, n_cap, g, sh, 0, o, nullptr, num_voxels, nullptr, workspace,
                    (hipStream_t)stream);
}
