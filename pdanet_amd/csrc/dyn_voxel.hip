// dyn_voxel.hip -- dynamic voxelization on the device (include/pda_train.h, pda_dyn_*): what the reference's DynamicMeanVFE
// and DynamicPillarVFE (pcdet/models/backbones_3d/vfe/dynamic_mean_vfe.py, dynamic_pillar_vfe.py) do with torch.unique and
// torch_scatter: every point inside the grid joins the voxel (or pillar) of its cell, no cap on voxels or points.
//
// pda_dyn_voxel_index, over the n rows of the collated points [batch_idx, x, y, z, ...]:
//   dv_keys          : key[i] = merge_coords of row i (voxel_cell.h gives the cells), DV_NONE for a row that joins nothing;
//                      the number of kept rows per tile of 256;
//   dv_scan          : one workgroup, exclusive scan of the tile counts; counts[0] = n_kept;
//   dv_compact       : point_idx = the kept rows in order (ballot / mbcnt ranks); (key, kept position) pairs for the sort;
//   dv_digit_count / dv_scan_digit / dv_digit_scatter (radix_sort.h), ceil(key_bits / 8) times: a stable LSD radix sort of the pairs, 8
//                      bits a pass: a digit histogram per tile of 2048 pairs, stored digit-major; one workgroup per digit
//                      scans its row of tiles, and the scatter adds the scan of the 256 digit totals, which gives every
//                      (digit, tile) its first output slot; the rank of a pair among the equal digits of its tile comes
//                      from 64-lane ballots (the lanes below with the same digit) and per-wave counts in LDS;
//   dv_head_count / dv_scan / dv_head_scatter : the first pair of every run of equal keys is a voxel; the scan of those
//                      flags is the rank of the key among the distinct keys (torch.unique sorts), counts[1] = n_voxels;
//                      the sort is stable, so the sorted kept positions are already the CSR lists in ascending point order;
//   dv_finish        : unq_cnt from seg_start, and zeros beyond the counts.
// Every grid depends on n alone, nothing is read back, and no result depends on the order threads run in: the only atomics
// are LDS integer adds into a histogram.  The reductions (pda_dyn_scatter_mean, pda_dyn_scatter_max_fwd) give one thread to
// a (voxel, column): the float32 sum has a fixed order, so its adds form one dependent chain whoever issues them, and what
// is left to spread over lanes are the loads -- neighbouring lanes read neighbouring columns of the same row, and the loop
// is unrolled so that four rows are in flight.  A thread walks one voxel, never a scene.
// The file is built with -ffp-contract=off.
#include "pda_common.h"
#include "radix_sort.h"
#include "voxel_cell.h"

namespace pda {
namespace {

constexpr uint32_t DV_NONE = 0xffffffffu;         // keys are below 2^31
constexpr int64_t DV_MAX_N = 1 << 30;
constexpr int DV_MAX_DIM = 1 << 24;               // (float)cells along an axis is exact
constexpr int DV_MAX_COLS = 256;


struct DynGrid {
    float lo[3], vs[3];
    int32_t n[3];      // cells along x, y, z
    int batch, pillars;
    uint32_t scale_b, scale_x, scale_y;      // merge_coords = b * scale_b + cx * scale_x + cy * scale_y + cz (pillars: cz = 0)
};


// The key of a row, DV_NONE when it joins nothing: a batch index outside [0, batch) (it is truncated as .int() does), a NaN
// among x, y, z, or a cell outside the grid (z is not tested for pillars).
__device__ __forceinline__ uint32_t key_of(const float* __restrict__ p, const DynGrid& g) {
    const float fb = p[0];
    if (is_nan_bits(fb) || !(fb > -1.f && fb < (float)g.batch)) return DV_NONE;
    if (is_nan_bits(p[3])) return DV_NONE;
    uint32_t cx, cy, cz = 0;
    if (!cell_axis(p[1], g.lo[0], g.vs[0], g.n[0], cx) || !cell_axis(p[2], g.lo[1], g.vs[1], g.n[1], cy)) return DV_NONE;
    if (!g.pillars && !cell_axis(p[3], g.lo[2], g.vs[2], g.n[2], cz)) return DV_NONE;
    return (uint32_t)(int)fb * g.scale_b + cx * g.scale_x + cy * g.scale_y + cz;
}


// ---- kept rows ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DV_TILE) void dv_keys(const float* __restrict__ pts, int n, int c1, DynGrid g,
                                                   uint32_t* __restrict__ key_raw, int32_t* __restrict__ tile_cnt) {
    const int i = blockIdx.x * DV_TILE + (int)threadIdx.x;
    uint32_t key = DV_NONE;
    if (i < n) {
        key = key_of(pts + (int64_t)i * c1, g);
        key_raw[i] = key;
    }
    store_tile_count(key != DV_NONE, tile_cnt + blockIdx.x);
}


// point_idx[pos] = the row of the pos-th kept point; the pair (key, pos) enters the sort.  Thread i also zeroes entry i of
// the point outputs when i lies beyond the kept count (nobody else writes there).
__global__ __launch_bounds__(DV_TILE) void dv_compact(int n, const uint32_t* __restrict__ key_raw,
                                                      const int32_t* __restrict__ tile_off, const int32_t* __restrict__ counts,
                                                      int32_t* __restrict__ point_idx, int32_t* __restrict__ unq_inv,
                                                      int32_t* __restrict__ seg_points, uint32_t* __restrict__ key,
                                                      int32_t* __restrict__ val) {
    const int i = blockIdx.x * DV_TILE + (int)threadIdx.x;
    const int nk = live(counts, 0, n);
    const uint32_t k = i < n ? key_raw[i] : DV_NONE;
    const bool keep = k != DV_NONE;
    const int pos = tile_off[blockIdx.x] + tile_rank_inclusive(keep) - 1;
    if (i < n && i >= nk) {
        point_idx[i] = 0;
        unq_inv[i] = 0;
        seg_points[i] = 0;
    }
    if (keep && pos < nk) {
        point_idx[pos] = i;
        key[pos] = k;
        val[pos] = pos;
    }
}


// ---- the voxels --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_head(const uint32_t* __restrict__ key, int j, int nk) {
    return j < nk && (j == 0 || key[j] != key[j - 1]);
}

__global__ __launch_bounds__(DV_TILE) void dv_head_count(int n, const int32_t* __restrict__ counts,
                                                         const uint32_t* __restrict__ key, int32_t* __restrict__ tile_cnt) {
    const int j = blockIdx.x * DV_TILE + (int)threadIdx.x;
    store_tile_count(is_head(key, j, live(counts, 0, n)), tile_cnt + blockIdx.x);
}

__global__ __launch_bounds__(DV_TILE) void dv_head_scatter(int n, DynGrid g, const int32_t* __restrict__ counts,
                                                           const uint32_t* __restrict__ key, const int32_t* __restrict__ val,
                                                           const int32_t* __restrict__ tile_off, int32_t* __restrict__ unq_inv,
                                                           int32_t* __restrict__ voxel_coords, int32_t* __restrict__ seg_start,
                                                           int32_t* __restrict__ seg_points) {
    const int j = blockIdx.x * DV_TILE + (int)threadIdx.x;
    const int nk = live(counts, 0, n), nv = live(counts, 1, n);
    const bool head = is_head(key, j, nk);
    const int v = tile_off[blockIdx.x] + tile_rank_inclusive(head) - 1;      // pair 0 is a head: v >= 0 for every pair
    if (j >= nk || v < 0 || v >= nv) return;
    const int pos = val[j];
    if (pos < 0 || pos >= nk) return;                                        // never, for a permutation of the kept positions
    unq_inv[pos] = v;
    seg_points[j] = pos;
    if (!head) return;
    seg_start[v] = j;
    uint32_t k = key[j];
    int32_t* cd = voxel_coords + (int64_t)v * 4;
    cd[0] = (int32_t)(k / g.scale_b);
    k %= g.scale_b;
    cd[3] = (int32_t)(k / g.scale_x);
    k %= g.scale_x;
    cd[2] = (int32_t)(k / g.scale_y);
    cd[1] = (int32_t)(k % g.scale_y);       // pillars: scale_y == 1, so 0
}

// unq_cnt, the closing entry of seg_start, and zeros beyond the voxel count.
__global__ __launch_bounds__(DV_TILE) void dv_finish(int n, const int32_t* __restrict__ counts, int32_t* __restrict__ unq_cnt,
                                                     int32_t* __restrict__ voxel_coords, int32_t* __restrict__ seg_start) {
    const int i = blockIdx.x * DV_TILE + (int)threadIdx.x;
    if (i >= n) return;
    const int nk = live(counts, 0, n), nv = live(counts, 1, n);
    if (i < nv) {
        const int end = i + 1 < nv ? seg_start[i + 1] : nk;
        unq_cnt[i] = end - seg_start[i];
        if (i + 1 == nv) seg_start[nv] = nk;      // read by no thread of this launch
    } else {
        unq_cnt[i] = 0;
        int32_t* cd = voxel_coords + (int64_t)i * 4;
        cd[0] = cd[1] = cd[2] = cd[3] = 0;
        seg_start[i + 1] = 0;
        if (i == 0) seg_start[0] = 0;             // no voxel at all
    }
}

// ---- the reductions ----------------------------------------------------------------------------------------------------
// out[v][f] = (the float32 sum of src[p][f] over the voxel's points p in ascending order) / float32(count).
__global__ __launch_bounds__(DV_TILE) void dv_scatter_mean(const float* __restrict__ src, int c, int64_t rows,
                                                           const int32_t* __restrict__ seg_start,
                                                           const int32_t* __restrict__ seg_points,
                                                           const int32_t* __restrict__ counts, float* __restrict__ out) {
    const int64_t id = (int64_t)blockIdx.x * DV_TILE + threadIdx.x;
    if (id >= rows * c) return;
    const int v = (int)(id / c), f = (int)(id % c);
    if (v >= live(counts, 1, rows)) {
        out[id] = 0.f;
        return;
    }
    const int s = seg_start[v], e = seg_start[v + 1];
    float acc = 0.f;
    int j = s;
    for (; j + 4 <= e; j += 4) {
        const float x0 = src[(int64_t)seg_points[j] * c + f], x1 = src[(int64_t)seg_points[j + 1] * c + f];
        const float x2 = src[(int64_t)seg_points[j + 2] * c + f], x3 = src[(int64_t)seg_points[j + 3] * c + f];
        acc = (((acc + x0) + x1) + x2) + x3;
    }
    for (; j < e; ++j) acc = acc + src[(int64_t)seg_points[j] * c + f];
    out[id] = acc / (float)(e - s);
}

// out[v][f] = the maximum of x[p][f] over the voxel's points, arg[v][f] = the lowest p that attains it (an update needs a
// strictly greater value, and the points come in ascending order).
__global__ __launch_bounds__(DV_TILE) void dv_scatter_max_fwd(const float* __restrict__ x, int c, int64_t rows,
                                                              const int32_t* __restrict__ seg_start,
                                                              const int32_t* __restrict__ seg_points,
                                                              const int32_t* __restrict__ counts, float* __restrict__ out,
                                                              int32_t* __restrict__ arg) {
    const int64_t id = (int64_t)blockIdx.x * DV_TILE + threadIdx.x;
    if (id >= rows * c) return;
    const int v = (int)(id / c), f = (int)(id % c);
    if (v >= live(counts, 1, rows)) {
        out[id] = 0.f;
        arg[id] = 0;
        return;
    }
    const int s = seg_start[v], e = seg_start[v + 1];
    int best = seg_points[s];
    float m = x[(int64_t)best * c + f];
    int j = s + 1;
    for (; j + 4 <= e; j += 4) {
        const int p0 = seg_points[j], p1 = seg_points[j + 1], p2 = seg_points[j + 2], p3 = seg_points[j + 3];
        const float x0 = x[(int64_t)p0 * c + f], x1 = x[(int64_t)p1 * c + f];
        const float x2 = x[(int64_t)p2 * c + f], x3 = x[(int64_t)p3 * c + f];
        if (x0 > m) { m = x0; best = p0; }
        if (x1 > m) { m = x1; best = p1; }
        if (x2 > m) { m = x2; best = p2; }
        if (x3 > m) { m = x3; best = p3; }
    }
    for (; j < e; ++j) {
        const int p = seg_points[j];
        const float xv = x[(int64_t)p * c + f];
        if (xv > m) { m = xv; best = p; }
    }
    out[id] = m;
    arg[id] = best;
}

// grad_x[p][f] = grad_out[v][f] where p is the argmax of its voxel v, else 0: a gather, one writer per entry.
__global__ __launch_bounds__(DV_TILE) void dv_scatter_max_bwd(const float* __restrict__ grad_out, const int32_t* __restrict__ arg,
                                                              const int32_t* __restrict__ unq_inv,
                                                              const int32_t* __restrict__ counts, int64_t rows, int64_t vox_rows,
                                                              int c, float* __restrict__ grad_x) {
    const int64_t id = (int64_t)blockIdx.x * DV_TILE + threadIdx.x;
    if (id >= rows * c) return;
    const int p = (int)(id / c), f = (int)(id % c);
    float g = 0.f;
    if (p < live(counts, 0, rows)) {
        const int v = unq_inv[p];
        if (v >= 0 && v < live(counts, 1, vox_rows) && arg[(int64_t)v * c + f] == p) g = grad_out[(int64_t)v * c + f];
    }
    grad_x[id] = g;
}

struct PillarArgs {
    float vs[3], off[3];
    int c1, absolute_xyz, with_distance, width;
};

// One thread per kept point: [points[:, 1:] or points[:, 4:], xyz - mean[voxel], xyz - cell centre, (|xyz|)].
__global__ __launch_bounds__(DV_TILE) void dv_pillar_features(const float* __restrict__ pts, int n, PillarArgs a,
                                                              const int32_t* __restrict__ point_idx,
                                                              const int32_t* __restrict__ unq_inv,
                                                              const int32_t* __restrict__ voxel_coords,
                                                              const float* __restrict__ mean, const int32_t* __restrict__ counts,
                                                              float* __restrict__ out) {
    const int i = blockIdx.x * DV_TILE + (int)threadIdx.x;
    if (i >= n) return;
    float* o = out + (int64_t)i * a.width;
    const int row = point_idx[i], v = unq_inv[i];
    if (i >= live(counts, 0, n) || row < 0 || row >= n || v < 0 || v >= live(counts, 1, n)) {
        for (int f = 0; f < a.width; ++f) o[f] = 0.f;
        return;
    }
    const float* p = pts + (int64_t)row * a.c1;
    const float x = p[1], y = p[2], z = p[3];
    int at = 0;
    for (int f = a.absolute_xyz ? 1 : 4; f < a.c1; ++f) o[at++] = p[f];
    const float* m = mean + (int64_t)v * 3;
    o[at++] = x - m[0];
    o[at++] = y - m[1];
    o[at++] = z - m[2];
    const int32_t* cd = voxel_coords + (int64_t)v * 4;
    o[at++] = x - ((float)cd[3] * a.vs[0] + a.off[0]);
    o[at++] = y - ((float)cd[2] * a.vs[1] + a.off[1]);
    o[at++] = z - a.off[2];
    // torch.norm on the CPU, which made the fixture: fused multiply-adds in column order (written out: -ffp-contract=off)
    if (a.with_distance) o[at++] = __builtin_sqrtf(__builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x)));
}

// ---- host --------------------------------------------------------------------------------------------------------------
int64_t pad256(int64_t x) { return (x + 255) / 256 * 256; }

struct Layout {
    int64_t key_a, key_b, val_a, val_b, tile_cnt, hist, digit_total, total;
};
Layout layout_of(int64_t n) {
    Layout l;
    int64_t at = 0;
    l.key_a = at; at += pad256(n * 4);
    l.key_b = at; at += pad256(n * 4);
    l.val_a = at; at += pad256(n * 4);
    l.val_b = at; at += pad256(n * 4);
    l.tile_cnt = at; at += pad256(divup64(n, DV_TILE) * 4);
    l.hist = at; at += pad256(sort_tiles_of(n) * DV_RADIX * 4);
    l.digit_total = at; at += pad256(DV_RADIX * 4);
    l.total = at;
    return l;
}

unsigned blocks_of(int64_t items) { return (unsigned)divup64(items, DV_TILE); }

bool reduce_sizes_ok(int64_t rows, int c) { return rows >= 0 && rows <= DV_MAX_N && c >= 1 && c <= DV_MAX_COLS; }

}  // namespace
}  // namespace pda

PDA_API int64_t pda_dyn_voxel_workspace_bytes(int64_t n, int key_bits) {
    if (n < 0 || n > pda::DV_MAX_N || key_bits < 1 || key_bits > 31) return -1;
    return pda::layout_of(n).total;
}

PDA_API int pda_dyn_voxel_index(const float* points, int64_t n, int c1, const float* range6, const float* voxel_size3,
                                const int32_t* grid3, int batch, int pillars, int32_t* counts, int32_t* point_idx,
                                int32_t* unq_inv, int32_t* unq_cnt, int32_t* voxel_coords, int32_t* seg_start,
                                int32_t* seg_points, void* workspace, pda_stream_t stream) {
    PDA_REQUIRE(n >= 0 && n <= pda::DV_MAX_N && c1 >= 4 && c1 <= pda::DV_MAX_COLS && batch >= 1 && batch <= (1 << 24) &&
                    (pillars == 0 || pillars == 1),
                "pda_dyn_voxel_index: bad size: n=%lld columns=%d batch=%d pillars=%d", (long long)n, c1, batch, pillars);
    PDA_REQUIRE(range6 && voxel_size3 && grid3, "pda_dyn_voxel_index: null pointer (range6 / voxel_size3 / grid3)");
    pda::DynGrid g;
    uint64_t cells = 1;
    const int axes = pillars ? 2 : 3;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = range6[a];
        g.vs[a] = voxel_size3[a];
        g.n[a] = grid3[a];
        PDA_REQUIRE(voxel_size3[a] > 0.f && voxel_size3[a] < 3.0e38f && grid3[a] >= 1 && grid3[a] <= pda::DV_MAX_DIM,
                    "pda_dyn_voxel_index: bad grid: voxel size %g, %d cells along axis %d (1 .. %d cells an axis)",
                    (double)voxel_size3[a], grid3[a], a, pda::DV_MAX_DIM);
        if (a < axes) cells *= (uint64_t)grid3[a];
        // the reference computes merge_coords in int32 and wraps silently from here on
        PDA_REQUIRE(cells * (uint64_t)batch < (1ull << 31),
                    "pda_dyn_voxel_index: key range: batch %d x grid %d x %d x %d%s reaches 2^31, the most an int32 merge_coords holds",
                    batch, grid3[0], grid3[1], grid3[2], pillars ? " (x, y)" : "");
    }
    if (n == 0) return PDA_OK;
    PDA_REQUIRE(points && counts && point_idx && unq_inv && unq_cnt && voxel_coords && seg_start && seg_points && workspace,
                "pda_dyn_voxel_index: null pointer");
    g.batch = batch;
    g.pillars = pillars;
    g.scale_y = pillars ? 1u : (uint32_t)grid3[2];
    g.scale_x = (uint32_t)grid3[1] * g.scale_y;
    g.scale_b = (uint32_t)grid3[0] * g.scale_x;
    const uint64_t range = cells * (uint64_t)batch;      // keys lie in [0, range)
    int key_bits = 1;
    while ((1ull << key_bits) < range) ++key_bits;

    const pda::Layout l = pda::layout_of(n);
    char* ws = (char*)workspace;
    uint32_t* key[2] = {(uint32_t*)(ws + l.key_a), (uint32_t*)(ws + l.key_b)};
    int32_t* val[2] = {(int32_t*)(ws + l.val_a), (int32_t*)(ws + l.val_b)};
    int32_t* tile_cnt = (int32_t*)(ws + l.tile_cnt);
    int32_t* hist = (int32_t*)(ws + l.hist);
    int32_t* digit_total = (int32_t*)(ws + l.digit_total);
    hipStream_t st = (hipStream_t)stream;
    const int ni = (int)n, tiles = (int)pda::divup64(n, pda::DV_TILE);
    const dim3 tgrid((unsigned)tiles), block(pda::DV_TILE);

    // the raw keys wait in key[1]: the first pass of the sort reads key[0] and overwrites them
    hipLaunchKernelGGL(pda::dv_keys, tgrid, block, 0, st, points, ni, c1, g, key[1], tile_cnt);
    hipLaunchKernelGGL(pda::dv_scan, dim3(1), dim3(1024), 0, st, tile_cnt, tiles, counts);
    hipLaunchKernelGGL(pda::dv_compact, tgrid, block, 0, st, ni, key[1], tile_cnt, counts, point_idx, unq_inv, seg_points, key[0],
                       val[0]);
    const int cur = pda::radix_sort_pairs(ni, key_bits, counts, key, val, hist, digit_total, st);
    hipLaunchKernelGGL(pda::dv_head_count, tgrid, block, 0, st, ni, counts, key[cur], tile_cnt);
    hipLaunchKernelGGL(pda::dv_scan, dim3(1), dim3(1024), 0, st, tile_cnt, tiles, counts + 1);
    hipLaunchKernelGGL(pda::dv_head_scatter, tgrid, block, 0, st, ni, g, counts, key[cur], val[cur], tile_cnt, unq_inv, voxel_coords,
                       seg_start, seg_points);
    hipLaunchKernelGGL(pda::dv_finish, tgrid, block, 0, st, ni, counts, unq_cnt, voxel_coords, seg_start);
    return pda::check_launch("pda_dyn_voxel_index");
}

PDA_API int pda_dyn_scatter_mean(const float* src, int c, const int32_t* seg_start, const int32_t* seg_points,
                                 const int32_t* counts, int64_t rows, float* out, pda_stream_t stream) {
    PDA_REQUIRE(pda::reduce_sizes_ok(rows, c), "pda_dyn_scatter_mean: bad size: rows=%lld columns=%d", (long long)rows, c);
    if (rows == 0) return PDA_OK;
    PDA_REQUIRE(src && seg_start && seg_points && counts && out, "pda_dyn_scatter_mean: null pointer");
    hipLaunchKernelGGL(pda::dv_scatter_mean, dim3(pda::blocks_of(rows * c)), dim3(pda::DV_TILE), 0, (hipStream_t)stream, src, c, rows,
                       seg_start, seg_points, counts, out);
    return pda::check_launch("pda_dyn_scatter_mean");
}

PDA_API int pda_dyn_scatter_max_fwd(const float* x, int c, const int32_t* seg_start, const int32_t* seg_points,
                                    const int32_t* counts, int64_t rows, float* out, int32_t* arg, pda_stream_t stream) {
    PDA_REQUIRE(pda::reduce_sizes_ok(rows, c), "pda_dyn_scatter_max_fwd: bad size: rows=%lld columns=%d", (long long)rows, c);
    if (rows == 0) return PDA_OK;
    PDA_REQUIRE(x && seg_start && seg_points && counts && out && arg, "pda_dyn_scatter_max_fwd: null pointer");
    hipLaunchKernelGGL(pda::dv_scatter_max_fwd, dim3(pda::blocks_of(rows * c)), dim3(pda::DV_TILE), 0, (hipStream_t)stream, x, c, rows,
                       seg_start, seg_points, counts, out, arg);
    return pda::check_launch("pda_dyn_scatter_max_fwd");
}

PDA_API int pda_dyn_scatter_max_bwd(const float* grad_out, const int32_t* arg, const int32_t* unq_inv, const int32_t* counts,
                                    int64_t rows, int64_t vox_rows, int c, float* grad_x, pda_stream_t stream) {
    PDA_REQUIRE(pda::reduce_sizes_ok(rows, c) && vox_rows >= 0 && vox_rows <= pda::DV_MAX_N,
                "pda_dyn_scatter_max_bwd: bad size: rows=%lld vox_rows=%lld columns=%d", (long long)rows, (long long)vox_rows, c);
    if (rows == 0) return PDA_OK;
    PDA_REQUIRE(arg && unq_inv && counts && grad_x && (grad_out || vox_rows == 0), "pda_dyn_scatter_max_bwd: null pointer");
    hipLaunchKernelGGL(pda::dv_scatter_max_bwd, dim3(pda::blocks_of(rows * c)), dim3(pda::DV_TILE), 0, (hipStream_t)stream, grad_out,
                       arg, unq_inv, counts, rows, vox_rows, c, grad_x);
    return pda::check_launch("pda_dyn_scatter_max_bwd");
}

PDA_API int pda_dyn_pillar_features(const float* points, int64_t n, int c1, const int32_t* point_idx, const int32_t* unq_inv,
                                    const int32_t* voxel_coords, const float* mean, const int32_t* counts,
                                    const float* voxel_size3, const float* offset3, int absolute_xyz, int with_distance,
                                    float* out, pda_stream_t stream) {
    PDA_REQUIRE(n >= 0 && n <= pda::DV_MAX_N && c1 >= 4 && c1 <= pda::DV_MAX_COLS && (absolute_xyz == 0 || absolute_xyz == 1) &&
                    (with_distance == 0 || with_distance == 1),
                "pda_dyn_pillar_features: bad size: n=%lld columns=%d absolute_xyz=%d with_distance=%d", (long long)n, c1,
                absolute_xyz, with_distance);
    PDA_REQUIRE(voxel_size3 && offset3, "pda_dyn_pillar_features: null pointer (voxel_size3 / offset3)");
    if (n == 0) return PDA_OK;
    PDA_REQUIRE(points && point_idx && unq_inv && voxel_coords && mean && counts && out, "pda_dyn_pillar_features: null pointer");
    pda::PillarArgs a;
    for (int k = 0; k < 3; ++k) {
        a.vs[k] = voxel_size3[k];
        a.off[k] = offset3[k];
    }
    a.c1 = c1;
    a.absolute_xyz = absolute_xyz;
    a.with_distance = with_distance;
    a.width = (absolute_xyz ? c1 - 1 : c1 - 4) + 6 + with_distance;
    hipLaunchKernelGGL(pda::dv_pillar_features, dim3(pda::blocks_of(n)), dim3(pda::DV_TILE), 0, (hipStream_t)stream, points, (int)n, a,
                       point_idx, unq_inv, voxel_coords, mean, counts, out);
    return pda::check_launch("pda_dyn_pillar_features");
}
