// sparse_conv_index.hip -- the index stage of the sparse 3D convolutions (include/pda_train.h, pda_spconv_index_*): which
// output sites a convolution has and which input row every (output row, tap) reads.  Coordinates only, never features.
//
// Both builds start alike, over the n rows (b, z, y, x) of the input:
//   sp_keys      : key[i] = ((b * D + z) * H + y) * W + x, SP_NONE for a row outside the grid (flag bit 1);
//   the sort     : (key, row) ascending, the stable radix sort of radix_sort.h; SP_NONE sorts behind every key;
//   sp_dups      : two equal neighbours in the sorted keys are a duplicate coordinate (flag bit 0).
// pda_spconv_index_subm then gives one thread to every (row, tap): the key of the neighbour, a binary search in the sorted
// keys, the row that holds it or -1.  A neighbour outside the grid is dropped before its key is formed, so nothing wraps into
// the next row, slice or scene.
// pda_spconv_index_strided:
//   sp_candidates: every input row emits the keys of the output sites whose window holds it, prod ceil(k_a / s_a) slots a row,
//                  SP_NONE in the slots that do not exist;
//   the sort, sp_head_count / dv_scan / sp_out_scatter: the distinct keys in ascending order are the output sites; stat[0]
//                  is their number, counted past `cap`; nothing is written from row `cap` on;
//   sp_nbr_out   : per (output row, tap) the input row at o * s - p + t, by binary search in the sorted input keys;
//   sp_nbr_in    : per (input row, tap) the output row o with o * s - p + t = the row's site, by binary search in the
//                  output keys.
// Only integer work; the atomics are integer adds in LDS (the sort's histogram) and integer ORs into the flag word, so two
// runs give the same bits.  Every grid is sized from n and cap alone; nothing is allocated or read back.
//
// The counted builds (pda_spconv_index_*_counted) are the same kernels with n a CAPACITY: the live rows are [0, *count_in), read
// on the device (`cnt` below; nullptr = all n rows).  Rows from *count_in on get the key SP_NONE, raise no flag, take part in
// no sort and no search, and their nbr rows are -1.  The count and the flags go to words of the workspace first; sp_finish
// writes count_out = min(found, cap), fills out_indices with -1 from there on and ORs the flags (and SP_FLAG_OVERFLOW) into
// the caller's status word, which is never cleared here.
#include "pda_common.h"
#include "radix_sort.h"

namespace pda {
namespace {

constexpr uint32_t SP_NONE = 0xffffffffu;      // keys are below 2^31
constexpr int64_t SP_MAX_ITEMS = 1 << 30;
constexpr int SP_MAX_K = 5;                    // taps along an axis
constexpr int SP_FLAG_DUPLICATE = 1, SP_FLAG_OUTSIDE = 2, SP_FLAG_OVERFLOW = 4;

struct SpGeom {
    int batch, T, cands;
    int in[3], out[3], k[3], s[3], p[3], cand[3];      // axes z, y, x
};

__device__ __forceinline__ bool in_grid(const int32_t* __restrict__ c, const SpGeom& g) {
    return c[0] >= 0 && c[0] < g.batch && c[1] >= 0 && c[1] < g.in[0] && c[2] >= 0 && c[2] < g.in[1] && c[3] >= 0 &&
           c[3] < g.in[2];
}
__device__ __forceinline__ uint32_t key_in(int b, int z, int y, int x, const SpGeom& g) {
    return (((uint32_t)b * (uint32_t)g.in[0] + (uint32_t)z) * (uint32_t)g.in[1] + (uint32_t)y) * (uint32_t)g.in[2] + (uint32_t)x;
}
__device__ __forceinline__ uint32_t key_out(int b, int z, int y, int x, const SpGeom& g) {
    return (((uint32_t)b * (uint32_t)g.out[0] + (uint32_t)z) * (uint32_t)g.out[1] + (uint32_t)y) * (uint32_t)g.out[2] + (uint32_t)x;
}
__device__ __forceinline__ void taps_of(int t, const SpGeom& g, int tap[3]) {
    tap[2] = t % g.k[2];
    t /= g.k[2];
    tap[1] = t % g.k[1];
    tap[0] = t / g.k[1];
}

// The position of `k` in the ascending a[0 .. n), -1 when it is absent (the first of equal entries).
__device__ __forceinline__ int find_key(const uint32_t* __restrict__ a, int n, uint32_t k) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo < n && a[lo] == k ? lo : -1;
}

__device__ __forceinline__ int live_in(const int32_t* __restrict__ cnt, int n) {
    if (cnt == nullptr) return n;
    const int32_t v = *cnt;
    return v < 0 ? 0 : (v > n ? n : v);
}

__device__ __forceinline__ int live_out(const int32_t* __restrict__ stat, int64_t cap) {
    const int32_t v = stat[0];
    return v < 0 ? 0 : (v > cap ? (int)cap : v);
}

__global__ __launch_bounds__(DV_TILE) void sp_keys(const int32_t* __restrict__ idx, int n, int m, SpGeom g,
                                                   uint32_t* __restrict__ key, int32_t* __restrict__ val,
                                                   int32_t* __restrict__ stat, int32_t* __restrict__ words,
                                                   const int32_t* __restrict__ cnt) {
    const int i = blockIdx.x * DV_TILE + (int)threadIdx.x;
    const int nl = live_in(cnt, n);
    if (i == 0) {
        words[0] = nl;      // the live pair counts the two sorts read
        words[1] = n > 0 ? nl * (m / n) : 0;
    }
    if (i >= n) return;
    const int32_t* c = idx + (int64_t)i * 4;
    const bool dead = i >= nl, ok = !dead && in_grid(c, g);
    key[i] = ok ? key_in(c[0], c[1], c[2], c[3], g) : SP_NONE;
    val[i] = i;
    if (!ok && !dead) atomicOr(stat + 1, SP_FLAG_OUTSIDE);
}

// The sorted pairs out of the sort's ping-pong buffers (the strided build sorts its candidates in them next).  A kernel and
// not two device-to-device copies, so that a captured counted build is made of kernel nodes only (see sp_clear).
__global__ __launch_bounds__(DV_TILE) void sp_keep_sorted(const uint32_t* __restrict__ key, const int32_t* __restrict__ val, int n,
                                                          uint32_t* __restrict__ skey, int32_t* __restrict__ srow) {
    const int i = blockIdx.x * DV_TILE + (int)threadIdx.x;
    if (i >= n) return;
    skey[i] = key[i];
    srow[i] = val[i];
}

__global__ __launch_bounds__(DV_TILE) void sp_dups(const uint32_t* __restrict__ skey, int n, int32_t* __restrict__ stat,
                                                   const int32_t* __restrict__ cnt) {
    const int j = blockIdx.x * DV_TILE + (int)threadIdx.x;
    if (j >= 1 && j < live_in(cnt, n) && skey[j] != SP_NONE && skey[j] == skey[j - 1]) atomicOr(stat + 1, SP_FLAG_DUPLICATE);
}

__global__ __launch_bounds__(DV_TILE) void sp_subm_nbr(const int32_t* __restrict__ idx, int n, SpGeom g,
                                                       const uint32_t* __restrict__ skey, const int32_t* __restrict__ srow,
                                                       int32_t* __restrict__ nbr, const int32_t* __restrict__ cnt) {
    const int64_t id = (int64_t)blockIdx.x * DV_TILE + threadIdx.x;
    if (id >= (int64_t)n * g.T) return;
    const int i = (int)(id / g.T);
    int tap[3];
    taps_of((int)(id % g.T), g, tap);
    const int32_t* c = idx + (int64_t)i * 4;
    int32_t r = -1;
    const int nl = live_in(cnt, n);
    if (i < nl && in_grid(c, g)) {
        const int z = c[1] + tap[0] - g.k[0] / 2, y = c[2] + tap[1] - g.k[1] / 2, x = c[3] + tap[2] - g.k[2] / 2;
        if (z >= 0 && z < g.in[0] && y >= 0 && y < g.in[1] && x >= 0 && x < g.in[2]) {
            const int pos = find_key(skey, nl, key_in(c[0], z, y, x, g));
            if (pos >= 0) r = srow[pos];
        }
    }
    nbr[id] = r;
}

__global__ __launch_bounds__(DV_TILE) void sp_candidates(const int32_t* __restrict__ idx, int n, SpGeom g,
                                                         uint32_t* __restrict__ key, int32_t* __restrict__ val,
                                                         const int32_t* __restrict__ cnt) {
    const int64_t id = (int64_t)blockIdx.x * DV_TILE + threadIdx.x;
    if (id >= (int64_t)n * g.cands) return;
    const int i = (int)(id / g.cands);
    int c = (int)(id % g.cands);
    int slot[3];
    slot[2] = c % g.cand[2];
    c /= g.cand[2];
    slot[1] = c % g.cand[1];
    slot[0] = c / g.cand[1];
    const int32_t* cd = idx + (int64_t)i * 4;
    bool ok = i < live_in(cnt, n) && in_grid(cd, g);
    int o[3] = {0, 0, 0};
    if (ok) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int v = cd[1 + a] + g.p[a];            // >= 0
            o[a] = v / g.s[a] - slot[a];                 // the window of o holds the site when 0 <= v - o * s < k
            ok = ok && o[a] >= 0 && o[a] < g.out[a] && v - o[a] * g.s[a] < g.k[a];
        }
    }
    key[id] = ok ? key_out(cd[0], o[0], o[1], o[2], g) : SP_NONE;
    val[id] = (int32_t)id;
}

__device__ __forceinline__ bool out_head(const uint32_t* __restrict__ key, int64_t j, int64_t m) {
    return j < m && key[j] != SP_NONE && (j == 0 || key[j] != key[j - 1]);
}

__global__ __launch_bounds__(DV_TILE) void sp_head_count(const uint32_t* __restrict__ key, int m, const int32_t* __restrict__ words,
                                                         int32_t* __restrict__ tile_cnt) {
    const int64_t j = (int64_t)blockIdx.x * DV_TILE + threadIdx.x;
    store_tile_count(out_head(key, j, live(words, 1, m)), tile_cnt + blockIdx.x);
}

__global__ __launch_bounds__(DV_TILE) void sp_out_scatter(const uint32_t* __restrict__ key, int m, const int32_t* __restrict__ words,
                                                          SpGeom g, int64_t cap, const int32_t* __restrict__ tile_off,
                                                          uint32_t* __restrict__ okey, int32_t* __restrict__ out_idx) {
    const int64_t j = (int64_t)blockIdx.x * DV_TILE + threadIdx.x;
    const bool head = out_head(key, j, live(words, 1, m));
    const int64_t r = (int64_t)tile_off[blockIdx.x] + tile_rank_inclusive(head) - 1;
    if (!head || r < 0 || r >= cap) return;
    uint32_t k = key[j];
    okey[r] = k;
    int32_t* o = out_idx + r * 4;
    o[3] = (int32_t)(k % (uint32_t)g.out[2]);
    k /= (uint32_t)g.out[2];
    o[2] = (int32_t)(k % (uint32_t)g.out[1]);
    k /= (uint32_t)g.out[1];
    o[1] = (int32_t)(k % (uint32_t)g.out[0]);
    o[0] = (int32_t)(k / (uint32_t)g.out[0]);
}

__global__ __launch_bounds__(DV_TILE) void sp_nbr_out(const uint32_t* __restrict__ okey, const int32_t* __restrict__ stat,
                                                      int64_t cap, int n, SpGeom g, const uint32_t* __restrict__ skey,
                                                      const int32_t* __restrict__ srow, int32_t* __restrict__ nbr,
                                                      const int32_t* __restrict__ cnt) {
    const int64_t id = (int64_t)blockIdx.x * DV_TILE + threadIdx.x;
    if (id >= cap * g.T) return;
    const int64_t o = id / g.T;
    int32_t r = -1;
    if (o < live_out(stat, cap)) {
        int tap[3];
        taps_of((int)(id % g.T), g, tap);
        uint32_t k = okey[o];
        const int ox = (int)(k % (uint32_t)g.out[2]);
        k /= (uint32_t)g.out[2];
        const int oy = (int)(k % (uint32_t)g.out[1]);
        k /= (uint32_t)g.out[1];
        const int oz = (int)(k % (uint32_t)g.out[0]), b = (int)(k / (uint32_t)g.out[0]);
        const int z = oz * g.s[0] - g.p[0] + tap[0], y = oy * g.s[1] - g.p[1] + tap[1], x = ox * g.s[2] - g.p[2] + tap[2];
        if (b < g.batch && z >= 0 && z < g.in[0] && y >= 0 && y < g.in[1] && x >= 0 && x < g.in[2]) {
            const int pos = find_key(skey, live_in(cnt, n), key_in(b, z, y, x, g));
            if (pos >= 0) r = srow[pos];
        }
    }
    nbr[id] = r;
}

__global__ __launch_bounds__(DV_TILE) void sp_nbr_in(const int32_t* __restrict__ idx, int n, SpGeom g,
                                                     const uint32_t* __restrict__ okey, const int32_t* __restrict__ stat,
                                                     int64_t cap, int32_t* __restrict__ nbr, const int32_t* __restrict__ cnt) {
    const int64_t id = (int64_t)blockIdx.x * DV_TILE + threadIdx.x;
    if (id >= (int64_t)n * g.T) return;
    const int i = (int)(id / g.T);
    int tap[3];
    taps_of((int)(id % g.T), g, tap);
    const int32_t* cd = idx + (int64_t)i * 4;
    bool ok = i < live_in(cnt, n) && in_grid(cd, g);
    int o[3] = {0, 0, 0};
    if (ok) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int v = cd[1 + a] + g.p[a] - tap[a];
            ok = ok && v >= 0 && v % g.s[a] == 0 && v / g.s[a] < g.out[a];
            o[a] = v >= 0 ? v / g.s[a] : 0;
        }
    }
    nbr[id] = ok ? find_key(okey, live_out(stat, cap), key_out(cd[0], o[0], o[1], o[2], g)) : -1;
}

// The start of a counted build: the count and the flags of this build, kept in the workspace.  A kernel and not the memset of
// the compact form: with the memset inside a captured graph, the second replay found stale flags there (MI355X).
__global__ void sp_clear(int32_t* __restrict__ stat) {
    if (threadIdx.x < 2) stat[threadIdx.x] = 0;
}

// The end of a counted build: out_idx (cap, 4) = -1 from min(stat[0], cap) on, *count_out = that number, *status |= the
// flags of this build.  cap == 0 (the submanifold form): only the flags.
__global__ __launch_bounds__(DV_TILE) void sp_finish(const int32_t* __restrict__ stat, int64_t cap, int32_t* __restrict__ out_idx,
                                                     int32_t* __restrict__ count_out, int32_t* __restrict__ status) {
    const int64_t id = (int64_t)blockIdx.x * DV_TILE + threadIdx.x;
    const int nl = live_out(stat, cap);
    if (id == 0) {
        if (count_out) *count_out = nl;
        const int32_t flags = stat[1] | (count_out && stat[0] > cap ? SP_FLAG_OVERFLOW : 0);
        if (flags) atomicOr(status, flags);
    }
    if (id < cap * 4 && id >= (int64_t)nl * 4) out_idx[id] = -1;
}

// ---- host --------------------------------------------------------------------------------------------------------------
int64_t pad256(int64_t x) { return (x + 255) / 256 * 256; }

struct SpLayout {
    int64_t key_a, key_b, val_a, val_b, tile_cnt, hist, digit_total, skey, srow, okey, words, total;
};
SpLayout layout_of(int64_t n, int64_t cap, int64_t cands) {
    const int64_t m = n * cands;
    SpLayout l;
    int64_t at = 0;
    l.key_a = at; at += pad256(m * 4);
    l.key_b = at; at += pad256(m * 4);
    l.val_a = at; at += pad256(m * 4);
    l.val_b = at; at += pad256(m * 4);
    l.tile_cnt = at; at += pad256(divup64(m, DV_TILE) * 4);
    l.hist = at; at += pad256(sort_tiles_of(m) * DV_RADIX * 4);
    l.digit_total = at; at += pad256(DV_RADIX * 4);
    l.skey = at; at += pad256(n * 4);
    l.srow = at; at += pad256(n * 4);
    l.okey = at; at += pad256(cap * 4);
    l.words = at; at += 256;
    l.total = at;
    return l;
}

int bits_of(uint64_t range) {      // 2^bits > range, so SP_NONE (all ones) lies above every key in the bits the sort reads
    int bits = 1;
    while ((1ull << bits) <= range) ++bits;
    return bits > 32 ? 32 : bits;
}

unsigned blocks_of(int64_t items) { return (unsigned)divup64(items, DV_TILE); }

// Checks the sizes and fills g; `strided` == 0: the submanifold form (odd kernel, stride 1, padding k / 2, out = in).
int geom_of(const char* who, int64_t n, int batch, const int* in3, const int* k3, const int* s3, const int* p3, int strided,
            SpGeom& g) {
    PDA_REQUIRE(n >= 0 && n <= SP_MAX_ITEMS && batch >= 1, "%s: bad size: n=%lld batch=%d", who, (long long)n, batch);
    g.batch = batch;
    g.T = g.cands = 1;
    uint64_t cells_in = (uint64_t)batch, cells_out = (uint64_t)batch;
    for (int a = 0; a < 3; ++a) {
        PDA_REQUIRE(in3[a] >= 1 && k3[a] >= 1 && k3[a] <= SP_MAX_K && s3[a] >= 1 && s3[a] <= 8 && p3[a] >= 0 && p3[a] <= 8,
                    "%s: bad size: axis %d: %d cells, kernel %d (1 .. %d), stride %d, padding %d", who, a, in3[a], k3[a], SP_MAX_K,
                    s3[a], p3[a]);
        PDA_REQUIRE(strided || (k3[a] % 2 == 1), "%s: a submanifold kernel is odd, got %d along axis %d", who, k3[a], a);
        g.in[a] = in3[a];
        g.k[a] = k3[a];
        g.s[a] = s3[a];
        g.p[a] = p3[a];
        PDA_REQUIRE(in3[a] + 2 * p3[a] >= k3[a], "%s: bad size: axis %d: %d cells + 2 * %d padding < kernel %d", who, a, in3[a],
                    p3[a], k3[a]);
        g.out[a] = strided ? (in3[a] + 2 * p3[a] - k3[a]) / s3[a] + 1 : in3[a];
        g.cand[a] = (k3[a] + s3[a] - 1) / s3[a];
        g.T *= k3[a];
        g.cands *= g.cand[a];
        cells_in *= (uint64_t)in3[a];
        cells_out *= (uint64_t)g.out[a];
        PDA_REQUIRE(cells_in < (1ull << 31) && cells_out < (1ull << 31),
                    "%s: key range: batch %d x grid %d x %d x %d (or its output grid) reaches 2^31, the most an int32 key holds", who,
                    batch, in3[0], in3[1], in3[2]);
    }
    PDA_REQUIRE(n * (int64_t)g.cands <= SP_MAX_ITEMS && n * (int64_t)g.T <= (int64_t)1 << 40, "%s: bad size: n=%lld is too many rows",
                who, (long long)n);
    return PDA_OK;
}

// The sorted (key, row) pairs of the input into skey / srow, flags into stat[1].
void sort_input(const int32_t* indices, int n, int m, const SpGeom& g, const SpLayout& l, char* ws, int32_t* stat, hipStream_t st,
                const int32_t* cnt = nullptr) {
    uint32_t* key[2] = {(uint32_t*)(ws + l.key_a), (uint32_t*)(ws + l.key_b)};
    int32_t* val[2] = {(int32_t*)(ws + l.val_a), (int32_t*)(ws + l.val_b)};
    int32_t* words = (int32_t*)(ws + l.words);
    uint64_t cells = (uint64_t)g.batch * g.in[0] * g.in[1] * g.in[2];
    hipLaunchKernelGGL(sp_keys, dim3(blocks_of(n)), dim3(DV_TILE), 0, st, indices, n, m, g, key[0], val[0], stat, words, cnt);
    const int cur = radix_sort_pairs(n, bits_of(cells), words, key, val, (int32_t*)(ws + l.hist), (int32_t*)(ws + l.digit_total), st);
    hipLaunchKernelGGL(sp_keep_sorted, dim3(blocks_of(n)), dim3(DV_TILE), 0, st, (const uint32_t*)key[cur], (const int32_t*)val[cur], n,
                       (uint32_t*)(ws + l.skey), (int32_t*)(ws + l.srow));
    hipLaunchKernelGGL(sp_dups, dim3(blocks_of(n)), dim3(DV_TILE), 0, st, (const uint32_t*)(ws + l.skey), n, stat, cnt);
}

}  // namespace
}  // namespace pda

PDA_API int64_t pda_spconv_index_workspace_bytes(int64_t n, int64_t cap, int candidates) {
    if (n < 0 || cap < 0 || candidates < 1 || candidates > 125 || n * candidates > pda::SP_MAX_ITEMS || cap > pda::SP_MAX_ITEMS) return -1;
    return pda::layout_of(n, cap, candidates).total;
}

namespace pda {
namespace {

// Both submanifold builds.  status == nullptr: the compact form, stat (2) is the caller's and written whole.  Otherwise the
// counted form: cnt gives the live rows, the flags are ORed into *status.
int subm_build(const char* who, const int32_t* indices, int64_t n, const int32_t* cnt, int batch, int d, int h, int w, int kd, int kh,
               int kw, int32_t* nbr_out, int32_t* stat, int32_t* status, void* workspace, hipStream_t st) {
    const int in3[3] = {d, h, w}, k3[3] = {kd, kh, kw}, s3[3] = {1, 1, 1}, p3[3] = {kd / 2, kh / 2, kw / 2};
    SpGeom g;
    const int rc = geom_of(who, n, batch, in3, k3, s3, p3, 0, g);
    if (rc != PDA_OK) return rc;
    if (n == 0) return PDA_OK;
    PDA_REQUIRE(indices && nbr_out && (stat || status) && workspace && (status == nullptr) == (cnt == nullptr), "%s: null pointer", who);
    const SpLayout l = layout_of(n, 0, 1);
    char* ws = (char*)workspace;
    if (status) {
        stat = (int32_t*)(ws + l.words) + 2;
        hipLaunchKernelGGL(sp_clear, dim3(1), dim3(64), 0, st, stat);
    } else {
        (void)hipMemsetAsync(stat, 0, 8, st);
    }
    sort_input(indices, (int)n, (int)n, g, l, ws, stat, st, cnt);
    hipLaunchKernelGGL(sp_subm_nbr, dim3(blocks_of(n * g.T)), dim3(DV_TILE), 0, st, indices, (int)n, g, (const uint32_t*)(ws + l.skey),
                       (const int32_t*)(ws + l.srow), nbr_out, cnt);
    if (status)
        hipLaunchKernelGGL(sp_finish, dim3(1), dim3(DV_TILE), 0, st, (const int32_t*)stat, (int64_t)0, (int32_t*)nullptr,
                           (int32_t*)nullptr, status);
    return check_launch(who);
}

int strided_build(const char* who, const int32_t* indices, int64_t n, const int32_t* cnt, int batch, int d, int h, int w, int kd, int kh,
                  int kw, int sd, int sh, int sw, int pd, int ph, int pw, int64_t cap, int32_t* out_indices, int32_t* nbr_out,
                  int32_t* nbr_in, int32_t* stat, int32_t* count_out, int32_t* status, void* workspace, hipStream_t st) {
    const int in3[3] = {d, h, w}, k3[3] = {kd, kh, kw}, s3[3] = {sd, sh, sw}, p3[3] = {pd, ph, pw};
    SpGeom g;
    const int rc = geom_of(who, n, batch, in3, k3, s3, p3, 1, g);
    if (rc != PDA_OK) return rc;
    PDA_REQUIRE(cap >= 0 && cap <= SP_MAX_ITEMS, "%s: bad size: cap=%lld", who, (long long)cap);
    if (n == 0) return PDA_OK;
    const bool counted = status != nullptr;
    PDA_REQUIRE(indices && nbr_in && (stat || counted) && workspace && (cap == 0 || (out_indices && nbr_out)) &&
                    counted == (cnt != nullptr) && counted == (count_out != nullptr), "%s: null pointer", who);
    const int ni = (int)n, m = (int)(n * g.cands);
    const SpLayout l = layout_of(n, cap, g.cands);
    char* ws = (char*)workspace;
    uint32_t* key[2] = {(uint32_t*)(ws + l.key_a), (uint32_t*)(ws + l.key_b)};
    int32_t* val[2] = {(int32_t*)(ws + l.val_a), (int32_t*)(ws + l.val_b)};
    int32_t* tile_cnt = (int32_t*)(ws + l.tile_cnt);
    int32_t* words = (int32_t*)(ws + l.words);
    const uint32_t* skey = (const uint32_t*)(ws + l.skey);
    const int32_t* srow = (const int32_t*)(ws + l.srow);
    uint32_t* okey = (uint32_t*)(ws + l.okey);
    const dim3 block(DV_TILE);
    if (counted) {
        stat = words + 2;
        hipLaunchKernelGGL(sp_clear, dim3(1), dim3(64), 0, st, stat);
    } else {
        (void)hipMemsetAsync(stat, 0, 8, st);
    }
    sort_input(indices, ni, m, g, l, ws, stat, st, cnt);
    hipLaunchKernelGGL(sp_candidates, dim3(blocks_of(m)), block, 0, st, indices, ni, g, key[0], val[0], cnt);
    const uint64_t cells_out = (uint64_t)g.batch * g.out[0] * g.out[1] * g.out[2];
    const int cur = radix_sort_pairs(m, bits_of(cells_out), words + 1, key, val, (int32_t*)(ws + l.hist), (int32_t*)(ws + l.digit_total), st);
    const int tiles = (int)divup64(m, DV_TILE);
    hipLaunchKernelGGL(sp_head_count, dim3((unsigned)tiles), block, 0, st, key[cur], m, (const int32_t*)words, tile_cnt);
    hipLaunchKernelGGL(dv_scan, dim3(1), dim3(1024), 0, st, tile_cnt, tiles, stat);
    hipLaunchKernelGGL(sp_out_scatter, dim3((unsigned)tiles), block, 0, st, key[cur], m, (const int32_t*)words, g, cap, tile_cnt, okey,
                       out_indices);
    if (cap > 0)
        hipLaunchKernelGGL(sp_nbr_out, dim3(blocks_of(cap * g.T)), block, 0, st, okey, stat, cap, ni, g, skey, srow, nbr_out, cnt);
    hipLaunchKernelGGL(sp_nbr_in, dim3(blocks_of(n * g.T)), block, 0, st, indices, ni, g, okey, stat, cap, nbr_in, cnt);
    if (counted)
        hipLaunchKernelGGL(sp_finish, dim3(blocks_of(cap * 4 > 0 ? cap * 4 : 1)), block, 0, st, (const int32_t*)stat, cap, out_indices,
                           count_out, status);
    return check_launch(who);
}

}  // namespace
}  // namespace pda

PDA_API int pda_spconv_index_subm(const int32_t* indices, int64_t n, int batch, int d, int h, int w, int kd, int kh, int kw,
                                  int32_t* nbr_out, int32_t* stat, void* workspace, pda_stream_t stream) {
    return pda::subm_build("pda_spconv_index_subm", indices, n, nullptr, batch, d, h, w, kd, kh, kw, nbr_out, stat, nullptr, workspace,
                           (hipStream_t)stream);
}

PDA_API int pda_spconv_index_strided(const int32_t* indices, int64_t n, int batch, int d, int h, int w, int kd, int kh, int kw,
                                     int sd, int sh, int sw, int pd, int ph, int pw, int64_t cap, int32_t* out_indices,
                                     int32_t* nbr_out, int32_t* nbr_in, int32_t* stat, void* workspace, pda_stream_t stream) {
    return pda::strided_build("pda_spconv_index_strided", indices, n, nullptr, batch, d, h, w, kd, kh, kw, sd, sh, sw, pd, ph, pw, cap,
                              out_indices, nbr_out, nbr_in, stat, nullptr, nullptr, workspace, (hipStream_t)stream);
}

PDA_API int pda_spconv_index_subm_counted(const int32_t* indices, int64_t n, const int32_t* count_in, int batch, int d, int h, int w,
                                          int kd, int kh, int kw, int32_t* nbr_out, int32_t* status, void* workspace,
                                          pda_stream_t stream) {
    const char* who = "pda_spconv_index_subm_counted";
    PDA_REQUIRE(n < 0 || n == 0 || (count_in && status), "%s: null pointer", who);
    return pda::subm_build(who, indices, n, count_in, batch, d, h, w, kd, kh, kw, nbr_out, nullptr, status, workspace,
                           (hipStream_t)stream);
}

PDA_API int pda_spconv_index_strided_counted(const int32_t* indices, int64_t n, const int32_t* count_in, int batch, int d, int h,
                                             int w, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, int64_t cap,
                                             int32_t* out_indices, int32_t* nbr_out, int32_t* nbr_in, int32_t* count_out,
                                             int32_t* status, void* workspace, pda_stream_t stream) {
    const char* who = "pda_spconv_index_strided_counted";
    PDA_REQUIRE(n < 0 || n == 0 || cap < 0 || (count_in && status && count_out), "%s: null pointer", who);
    return pda::strided_build(who, indices, n, count_in, batch, d, h, w, kd, kh, kw, sd, sh, sw, pd, ph, pw, cap, out_indices, nbr_out,
                              nbr_in, nullptr, count_out, status, workspace, (hipStream_t)stream);
}
