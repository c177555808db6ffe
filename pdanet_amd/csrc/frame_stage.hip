// frame_stage.hip -- what happens to a raw frame before the augmentor sees it, on the device (include/pda_train.h,
// pda_kitti_fov_filter / pda_gt_extract_count / pda_gt_extract_write).
//
// pda_kitti_fov_filter: KittiDataset's FOV_POINTS_ONLY step (pcdet/datasets/kitti/kitti_dataset.py get_fov_flag behind
// calib.lidar_to_rect / calib.rect_to_img) for a batch of packed scenes.  Per point, in float32 without FMA (the file is
// built with -ffp-contract=off; the division is HIP's correctly rounded one):
//   rect_k = ((x*M[0][k] + y*M[1][k]) + z*M[2][k]) + M[3][k]            M = V2C^T R0^T (4, 3), formed by the caller
//   h_j    = ((rx*P2[j][0] + ry*P2[j][1]) + rz*P2[j][2]) + P2[j][3]
//   u = h_0 / rz, v = h_1 / rz, depth = h_2 - P2[2][3]
//   keep iff u >= 0 && u < W && v >= 0 && v < H && depth >= 0          (a NaN keeps nothing)
// followed by a stable ragged compaction shaped like the input stage's:
//   ff_count_kernel   (tiles, B): kept points per tile of 256;
//   ff_scan_kernel    (B)       : exclusive scan of a scene's tile counts in place, scene totals and status into info;
//   ff_offsets_kernel (1)       : exclusive scan of the scene totals into out_offsets;
//   ff_scatter_kernel (tiles, B): positions from the 64-bit ballot + mbcnt inside a wave, LDS across the waves, the scanned
//                                 tile offset across tiles; a row of C == 4 is one 16-byte load and one 16-byte store.
//
// pda_gt_extract_*: the body of create_groundtruth_database for a batch of frames: for every box, in box order, the
// points of its own frame inside it (the CPU test points_in_boxes_cpu: box_rec.h in_box_rec<false>, margin 1e-2), in point
// order, shifted by the box centre in double.  Per workgroup the frame's box records are staged through LDS once, then
// every tile's ballots (wave, box) are kept in LDS:
//   gx_count_kernel (tile groups, B): per (box, tile) counts from the ballots;
//   gx_scan_kernel  (256, B)        : per box, the exclusive scan of its tile counts in place and its total into counts;
//   gx_write_kernel (tile groups, B): the same ballots again; a row's position is the object's offset + the scanned tile
//                                     offset + the waves before + mbcnt.  No atomics decide an order.
#include "pda_common.h"
#include "ragged_scene.h"
#include "box_rec.h"

namespace pda {
namespace {

constexpr int FS_TILE = 256;
constexpr int FS_WAVES = FS_TILE / PDA_WAVE;
constexpr int GX_MAX_BOXES = 256;   // boxes of one frame (LDS staging)
constexpr int GX_GROUP = 4;         // tiles one workgroup walks with the records staged once
// info[b][3] status bit of this stage (include/pda_train.h), next to ragged_scene.h's
constexpr int ST_OVER_BOXES = 8;

// cal: 24 floats, M (4, 3) row-major then P2 (3, 4) row-major, wave-uniform (scalar loads)
__device__ __forceinline__ bool fov_keep(float x, float y, float z, cfloat_ptr cal, double hh, double ww) {
    const float rx = ((x * cal[0] + y * cal[3]) + z * cal[6]) + cal[9];
    const float ry = ((x * cal[1] + y * cal[4]) + z * cal[7]) + cal[10];
    const float rz = ((x * cal[2] + y * cal[5]) + z * cal[8]) + cal[11];
    const float h0 = ((rx * cal[12] + ry * cal[13]) + rz * cal[14]) + cal[15];
    const float h1 = ((rx * cal[16] + ry * cal[17]) + rz * cal[18]) + cal[19];
    const float h2 = ((rx * cal[20] + ry * cal[21]) + rz * cal[22]) + cal[23];
    const float u = h0 / rz, v = h1 / rz, depth = h2 - cal[23];
    if (is_nan_bits(u) || is_nan_bits(v) || is_nan_bits(depth)) return false;
    return u >= 0.f && (double)u < ww && v >= 0.f && (double)v < hh && depth >= 0.f;
}

template <bool VEC4>
__device__ __forceinline__ bool ff_flag(const float* __restrict__ pts, const Scene& s, int i, int c, cfloat_ptr cal, double hh,
                                        double ww, float4& row) {
    if (i >= s.n) return false;
    const float* p = pts + (s.start + i) * (int64_t)c;
    if (VEC4) {
        row = load4(p);
    } else {
        row.x = p[0];
        row.y = p[1];
        row.z = p[2];
    }
    return fov_keep(row.x, row.y, row.z, cal, hh, ww);
}

// ---- the FOV filter ----------------------------------------------------------------------------------------------------
template <bool VEC4>
__global__ __launch_bounds__(FS_TILE) void ff_count_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off,
                                                           int64_t n_total, int c, int64_t n_cap,
                                                           const float* __restrict__ calib, const int32_t* __restrict__ shape,
                                                           int tiles, int32_t* __restrict__ tile_cnt) {
    __shared__ int32_t wk[FS_WAVES];
    const int b = blockIdx.y, t = blockIdx.x;
    const Scene s = scene_of(off, b, n_total, n_cap);
    float4 row;
    const bool keep = ff_flag<VEC4>(pts, s, t * FS_TILE + (int)threadIdx.x, c, as_constant(calib + (int64_t)b * 24),
                                    (double)shape[b * 2], (double)shape[b * 2 + 1], row);
    const uint64_t bk = __ballot(keep);
    if (lane_id() == 0) wk[wave_id()] = __popcll(bk);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t sum = 0;
        for (int w = 0; w < FS_WAVES; ++w) sum += wk[w];
        tile_cnt[(int64_t)b * tiles + t] = sum;
    }
}

// One workgroup per scene.  Thread u owns the `per` consecutive tiles from u * per.
__global__ __launch_bounds__(1024) void ff_scan_kernel(const int64_t* __restrict__ off, int64_t n_total, int64_t n_cap, int tiles,
                                                       int32_t* __restrict__ tile_cnt, int32_t* __restrict__ info) {
    __shared__ int32_t ps[1024];
    const int b = blockIdx.x, u = threadIdx.x;
    const int per = (tiles + 1023) / 1024;
    const int t0 = min(tiles, u * per), t1 = min(tiles, t0 + per);
    int32_t* tc = tile_cnt + (int64_t)b * tiles;
    int32_t sum = 0;
    for (int t = t0; t < t1; ++t) sum += tc[t];
    ps[u] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {          // Hillis-Steele inclusive scan of the 1024 partial sums
        const int32_t v = u >= o ? ps[u - o] : 0;
        __syncthreads();
        ps[u] += v;
        __syncthreads();
    }
    int32_t r = ps[u] - sum;
    for (int t = t0; t < t1; ++t) {
        const int32_t cnt = tc[t];
        tc[t] = r;
        r += cnt;
    }
    if (u == 1023) {
        const Scene s = scene_of(off, b, n_total, n_cap);
        info[b * 4 + 0] = s.n;
        info[b * 4 + 1] = ps[1023];
        info[b * 4 + 2] = 0;
        info[b * 4 + 3] = s.status;
    }
}

// out_offsets (batch + 1) = the exclusive scan of info[:, 1].  One workgroup; thread u owns `per` consecutive scenes.
__global__ __launch_bounds__(1024) void ff_offsets_kernel(const int32_t* __restrict__ info, int batch,
                                                          int64_t* __restrict__ out_offsets) {
    __shared__ int64_t ps[1024];
    const int u = threadIdx.x;
    const int per = (batch + 1023) / 1024;
    const int b0 = min(batch, u * per), b1 = min(batch, b0 + per);
    int64_t sum = 0;
    for (int b = b0; b < b1; ++b) sum += info[b * 4 + 1];
    ps[u] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t v = u >= o ? ps[u - o] : 0;
        __syncthreads();
        ps[u] += v;
        __syncthreads();
    }
    int64_t r = ps[u] - sum;
    for (int b = b0; b < b1; ++b) {
        out_offsets[b] = r;
        r += info[b * 4 + 1];
    }
    if (u == 1023) out_offsets[batch] = ps[1023];
}

template <bool VEC4>
__global__ __launch_bounds__(FS_TILE) void ff_scatter_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off,
                                                             int64_t n_total, int c, int64_t n_cap,
                                                             const float* __restrict__ calib, const int32_t* __restrict__ shape,
                                                             int tiles, const int32_t* __restrict__ tile_off,
                                                             const int64_t* __restrict__ out_offsets, float* __restrict__ out,
                                                             int64_t out_cap, int32_t* __restrict__ info) {
    __shared__ int32_t wk[FS_WAVES];
    const int b = blockIdx.y, t = blockIdx.x;
    const Scene s = scene_of(off, b, n_total, n_cap);
    const int i = t * FS_TILE + (int)threadIdx.x;
    float4 row;
    const bool keep = ff_flag<VEC4>(pts, s, i, c, as_constant(calib + (int64_t)b * 24), (double)shape[b * 2],
                                    (double)shape[b * 2 + 1], row);
    const uint64_t bk = __ballot(keep);
    const int w = wave_id();
    if (lane_id() == 0) wk[w] = __popcll(bk);
    __syncthreads();
    if (!keep) return;
    int64_t pos = out_offsets[b] + tile_off[(int64_t)b * tiles + t] + rank_below(bk);
    for (int v = 0; v < w; ++v) pos += wk[v];
    if (pos < 0 || pos >= out_cap) {              // overlapping scenes can keep more rows than the buffer holds
        atomicOr(info + b * 4 + 3, ST_OVER_CAP);
        return;
    }
    float* o = out + pos * (int64_t)c;
    if (VEC4) {
        store4(o, row);
    } else {
        const float* p = pts + (s.start + i) * (int64_t)c;
        for (int f = 0; f < c; ++f) o[f] = p[f];
    }
}

// ---- the gt database extraction -------------------------------------------------------------------------------------------
struct Frame {
    Scene pts;
    int64_t bstart;
    int nb;        // boxes this frame holds (0 when the frame is unusable)
    int nb_raw;    // what its box offsets say (clamped to int)
    int status;
};

__device__ __forceinline__ Frame frame_of(const int64_t* __restrict__ off, const int64_t* __restrict__ boff, int b,
                                          int64_t n_total, int64_t n_cap, int64_t m_total) {
    Frame f;
    f.pts = scene_of(off, b, n_total, n_cap);
    f.status = f.pts.status;
    f.bstart = 0;
    f.nb = f.nb_raw = 0;
    const int64_t s = boff[b], e = boff[b + 1];
    if (s < 0 || e < s || e > m_total) {
        f.status |= ST_BAD_OFFSETS;
    } else {
        f.nb_raw = (int)min(e - s, (int64_t)INT32_MAX);
        if (e - s > GX_MAX_BOXES) f.status |= ST_OVER_BOXES;
        else { f.bstart = s; f.nb = (int)(e - s); }
    }
    if (f.status) {        // a frame with any status is written empty
        f.nb = 0;
        f.pts.n = 0;
    }
    return f;
}

__device__ __forceinline__ void gx_stage_boxes(const float* __restrict__ boxes, const Frame& f, BoxRec* rec) {
    for (int j = threadIdx.x; j < f.nb; j += FS_TILE) {
        const float* bx = boxes + (f.bstart + j) * 7;
        rec[j] = make_box_rec(bx[0], bx[1], bx[2], bx[3], bx[4], bx[5], bx[6], (double)1e-2f);
    }
}

// the ballots of one tile: ball[w][j] = the lanes of wave w whose point lies in box j
__device__ __forceinline__ void gx_tile_ballots(bool have, float x, float y, float z, const BoxRec* rec, int nb,
                                                uint64_t (*ball)[GX_MAX_BOXES]) {
    const int w = wave_id();
    for (int j = 0; j < nb; ++j) {
        const uint64_t bm = __ballot(have && in_box_rec<false>(rec[j], x, y, z));
        if (lane_id() == 0) ball[w][j] = bm;
    }
}

__global__ __launch_bounds__(FS_TILE) void gx_count_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off,
                                                           int64_t n_total, int c, int64_t n_cap,
                                                           const float* __restrict__ boxes, const int64_t* __restrict__ boff,
                                                           int64_t m_total, int tiles, int32_t* __restrict__ tile_cnt) {
    __shared__ BoxRec rec[GX_MAX_BOXES];
    __shared__ uint64_t ball[FS_WAVES][GX_MAX_BOXES];
    const int b = blockIdx.y;
    const Frame f = frame_of(off, boff, b, n_total, n_cap, m_total);
    if (f.nb == 0) return;
    gx_stage_boxes(boxes, f, rec);
    __syncthreads();
    for (int g = 0; g < GX_GROUP; ++g) {
        const int t = blockIdx.x * GX_GROUP + g;
        if (t >= tiles) break;
        const int i = t * FS_TILE + (int)threadIdx.x;
        const bool have = i < f.pts.n;
        float x = 0.f, y = 0.f, z = 0.f;
        if (have) {
            const float* p = pts + (f.pts.start + i) * (int64_t)c;
            x = p[0];
            y = p[1];
            z = p[2];
        }
        gx_tile_ballots(have, x, y, z, rec, f.nb, ball);
        __syncthreads();
        for (int j = threadIdx.x; j < f.nb; j += FS_TILE) {
            int32_t sum = 0;
            for (int w = 0; w < FS_WAVES; ++w) sum += __popcll(ball[w][j]);
            tile_cnt[(f.bstart + j) * tiles + t] = sum;
        }
        __syncthreads();
    }
}

// Workgroup (j, b): box j of frame b.  Thread u owns `per` consecutive tiles.  Workgroup (0, b) also writes info[b].
__global__ __launch_bounds__(FS_TILE) void gx_scan_kernel(const int64_t* __restrict__ off, const int64_t* __restrict__ boff,
                                                          int64_t n_total, int64_t n_cap, int64_t m_total, int tiles,
                                                          int32_t* __restrict__ tile_cnt, int32_t* __restrict__ counts,
                                                          int32_t* __restrict__ info) {
    __shared__ int32_t ps[FS_TILE];
    const int b = blockIdx.y, j = blockIdx.x, u = threadIdx.x;
    const Frame f = frame_of(off, boff, b, n_total, n_cap, m_total);
    if (j == 0 && u == 0) {
        info[b * 4 + 0] = f.pts.n;
        info[b * 4 + 1] = f.nb_raw;
        info[b * 4 + 2] = 0;
        info[b * 4 + 3] = f.status;
    }
    if (j >= f.nb) return;
    const int per = (tiles + FS_TILE - 1) / FS_TILE;
    const int t0 = min(tiles, u * per), t1 = min(tiles, t0 + per);
    int32_t* tc = tile_cnt + (f.bstart + j) * tiles;
    int32_t sum = 0;
    for (int t = t0; t < t1; ++t) sum += tc[t];
    ps[u] = sum;
    __syncthreads();
    for (int o = 1; o < FS_TILE; o <<= 1) {
        const int32_t v = u >= o ? ps[u - o] : 0;
        __syncthreads();
        ps[u] += v;
        __syncthreads();
    }
    int32_t r = ps[u] - sum;
    for (int t = t0; t < t1; ++t) {
        const int32_t cnt = tc[t];
        tc[t] = r;
        r += cnt;
    }
    if (u == FS_TILE - 1) counts[f.bstart + j] = ps[FS_TILE - 1];
}

template <bool VEC4>
__global__ __launch_bounds__(FS_TILE) void gx_write_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off,
                                                           int64_t n_total, int c, int64_t n_cap,
                                                           const float* __restrict__ boxes, const int64_t* __restrict__ boff,
                                                           int64_t m_total, const double* __restrict__ centre,
                                                           const int64_t* __restrict__ obj_off, int tiles,
                                                           const int32_t* __restrict__ tile_off, float* __restrict__ out,
                                                           int64_t out_cap, int32_t* __restrict__ info) {
    __shared__ BoxRec rec[GX_MAX_BOXES];
    __shared__ uint64_t ball[FS_WAVES][GX_MAX_BOXES];
    __shared__ double ctr[GX_MAX_BOXES][3];
    __shared__ int64_t obeg[GX_MAX_BOXES], oend[GX_MAX_BOXES];
    const int b = blockIdx.y;
    const Frame f = frame_of(off, boff, b, n_total, n_cap, m_total);
    if (f.nb == 0) return;
    gx_stage_boxes(boxes, f, rec);
    for (int j = threadIdx.x; j < f.nb; j += FS_TILE) {
        const int64_t g = f.bstart + j;
        ctr[j][0] = centre[g * 3 + 0];
        ctr[j][1] = centre[g * 3 + 1];
        ctr[j][2] = centre[g * 3 + 2];
        obeg[j] = obj_off[g];
        oend[j] = min(obj_off[g + 1], out_cap);
    }
    __syncthreads();
    const int w = wave_id();
    for (int g = 0; g < GX_GROUP; ++g) {
        const int t = blockIdx.x * GX_GROUP + g;
        if (t >= tiles) break;
        const int i = t * FS_TILE + (int)threadIdx.x;
        const bool have = i < f.pts.n;
        float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
        const float* p = pts + (f.pts.start + (have ? i : 0)) * (int64_t)c;
        if (have) {
            if (VEC4) {
                row = load4(p);
            } else {
                row.x = p[0];
                row.y = p[1];
                row.z = p[2];
            }
        }
        gx_tile_ballots(have, row.x, row.y, row.z, rec, f.nb, ball);
        __syncthreads();
        for (int j = 0; j < f.nb; ++j) {
            const uint64_t mine = ball[w][j];
            if (mine == 0) continue;                       // wave-uniform
            if (!((mine >> lane_id()) & 1)) continue;
            int64_t pos = obeg[j] + tile_off[(f.bstart + j) * tiles + t] + rank_below(mine);
            for (int v = 0; v < w; ++v) pos += __popcll(ball[v][j]);
            if (obeg[j] < 0 || pos < obeg[j] || pos >= oend[j]) {   // the offsets do not hold what was counted
                atomicOr(info + b * 4 + 3, ST_OVER_CAP);
                continue;
            }
            float* o = out + pos * (int64_t)c;
            const float sx = (float)((double)row.x - ctr[j][0]);
            const float sy = (float)((double)row.y - ctr[j][1]);
            const float sz = (float)((double)row.z - ctr[j][2]);
            if (VEC4) {
                store4(o, make_float4(sx, sy, sz, row.w));
            } else {
                o[0] = sx;
                o[1] = sy;
                o[2] = sz;
                for (int q = 3; q < c; ++q) o[q] = p[q];
            }
        }
        __syncthreads();
    }
}

int64_t tiles_of(int64_t n_cap) { return divup64(n_cap, FS_TILE); }
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
int64_t gx_bytes(int64_t m_total, int64_t n_cap) { return (m_total * tiles_of(n_cap) * 4 + 255) / 256 * 256; }
bool gx_sizes_ok(int batch, int64_t n_cap, int64_t m_total) {
    return stage_sizes_ok(batch, n_cap) && m_total >= 0 && m_total <= (1 << 24) && gx_bytes(m_total, n_cap) <= ((int64_t)1 << 36);
}

}  // namespace
}  // namespace pda

PDA_API int64_t pda_kitti_fov_filter_workspace_bytes(int batch, int64_t n_cap) {
    if (!pda::stage_sizes_ok(batch, n_cap)) return -1;
    return (batch * pda::tiles_of(n_cap) * 4 + 255) / 256 * 256;
}

PDA_API int pda_kitti_fov_filter(const float* points, const int64_t* offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                                 const float* calib, const int32_t* image_shape, float* out_points, int64_t out_cap,
                                 int64_t* out_offsets, int32_t* info, void* workspace, pda_stream_t stream) {
    PDA_REQUIRE(pda::stage_sizes_ok(batch, n_cap) && n_total >= 0 && c >= 3 && c <= 64 && out_cap >= 0,
                "pda_kitti_fov_filter: bad size: batch=%d n_total=%lld C=%d n_cap=%lld out_cap=%lld", batch, (long long)n_total, c,
                (long long)n_cap, (long long)out_cap);
    if (batch == 0) return PDA_OK;
    PDA_REQUIRE(offsets && calib && image_shape && out_offsets && info && workspace && (points || n_total == 0) &&
                    (out_points || out_cap == 0),
                "pda_kitti_fov_filter: null pointer");
    const int tiles = (int)pda::tiles_of(n_cap);
    int32_t* tile_cnt = (int32_t*)workspace;
    hipStream_t st = (hipStream_t)stream;
    const dim3 tgrid((unsigned)tiles, (unsigned)batch);
    const bool vec4 = c == 4 && pda::aligned16(points) && pda::aligned16(out_points);
    if (vec4)
        hipLaunchKernelGGL(pda::ff_count_kernel<true>, tgrid, dim3(pda::FS_TILE), 0, st, points, offsets, n_total, c, n_cap, calib,
                           image_shape, tiles, tile_cnt);
    else
        hipLaunchKernelGGL(pda::ff_count_kernel<false>, tgrid, dim3(pda::FS_TILE), 0, st, points, offsets, n_total, c, n_cap, calib,
                           image_shape, tiles, tile_cnt);
    hipLaunchKernelGGL(pda::ff_scan_kernel, dim3((unsigned)batch), dim3(1024), 0, st, offsets, n_total, n_cap, tiles, tile_cnt, info);
    hipLaunchKernelGGL(pda::ff_offsets_kernel, dim3(1), dim3(1024), 0, st, info, batch, out_offsets);
    if (vec4)
        hipLaunchKernelGGL(pda::ff_scatter_kernel<true>, tgrid, dim3(pda::FS_TILE), 0, st, points, offsets, n_total, c, n_cap, calib,
                           image_shape, tiles, tile_cnt, out_offsets, out_points, out_cap, info);
    else
        hipLaunchKernelGGL(pda::ff_scatter_kernel<false>, tgrid, dim3(pda::FS_TILE), 0, st, points, offsets, n_total, c, n_cap, calib,
                           image_shape, tiles, tile_cnt, out_offsets, out_points, out_cap, info);
    return pda::check_launch("pda_kitti_fov_filter");
}

PDA_API int64_t pda_gt_extract_workspace_bytes(int batch, int64_t n_cap, int64_t m_total) {
    if (!pda::gx_sizes_ok(batch, n_cap, m_total)) return -1;
    return pda::gx_bytes(m_total, n_cap);
}

PDA_API int pda_gt_extract_count(const float* points, const int64_t* offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                                 const float* boxes, const int64_t* box_offsets, int64_t m_total, int32_t* counts, int32_t* info,
                                 void* workspace, pda_stream_t stream) {
    PDA_REQUIRE(pda::gx_sizes_ok(batch, n_cap, m_total) && n_total >= 0 && c >= 3 && c <= 64,
                "pda_gt_extract_count: bad size: batch=%d n_total=%lld C=%d n_cap=%lld m_total=%lld", batch, (long long)n_total, c,
                (long long)n_cap, (long long)m_total);
    if (batch == 0) return PDA_OK;
    PDA_REQUIRE(offsets && box_offsets && info && (points || n_total == 0) && ((boxes && counts && workspace) || m_total == 0),
                "pda_gt_extract_count: null pointer");
    const int tiles = (int)pda::tiles_of(n_cap);
    hipStream_t st = (hipStream_t)stream;
    if (m_total > 0) (void)hipMemsetAsync(counts, 0, (size_t)m_total * 4, st);   // boxes of unusable frames count 0
    hipLaunchKernelGGL(pda::gx_count_kernel, dim3((unsigned)pda::divup(tiles, pda::GX_GROUP), (unsigned)batch), dim3(pda::FS_TILE), 0,
                       st, points, offsets, n_total, c, n_cap, boxes, box_offsets, m_total, tiles, (int32_t*)workspace);
    hipLaunchKernelGGL(pda::gx_scan_kernel, dim3((unsigned)pda::GX_MAX_BOXES, (unsigned)batch), dim3(pda::FS_TILE), 0, st, offsets,
                       box_offsets, n_total, n_cap, m_total, tiles, (int32_t*)workspace, counts, info);
    return pda::check_launch("pda_gt_extract_count");
}

PDA_API int pda_gt_extract_write(const float* points, const int64_t* offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                                 const float* boxes, const int64_t* box_offsets, int64_t m_total, const double* centre,
                                 const int64_t* obj_offsets, float* obj_points, int64_t out_cap, int32_t* info, void* workspace,
                                 pda_stream_t stream) {
    PDA_REQUIRE(pda::gx_sizes_ok(batch, n_cap, m_total) && n_total >= 0 && c >= 3 && c <= 64 && out_cap >= 0,
                "pda_gt_extract_write: bad size: batch=%d n_total=%lld C=%d n_cap=%lld m_total=%lld out_cap=%lld", batch,
                (long long)n_total, c, (long long)n_cap, (long long)m_total, (long long)out_cap);
    if (batch == 0 || m_total == 0) return PDA_OK;
    PDA_REQUIRE(offsets && box_offsets && info && boxes && centre && obj_offsets && workspace && (points || n_total == 0) &&
                    (obj_points || out_cap == 0),
                "pda_gt_extract_write: null pointer");
    const int tiles = (int)pda::tiles_of(n_cap);
    const dim3 grid((unsigned)pda::divup(tiles, pda::GX_GROUP), (unsigned)batch);
    if (c == 4 && pda::aligned16(points) && pda::aligned16(obj_points))
        hipLaunchKernelGGL(pda::gx_write_kernel<true>, grid, dim3(pda::FS_TILE), 0, (hipStream_t)stream, points, offsets, n_total, c,
                           n_cap, boxes, box_offsets, m_total, centre, obj_offsets, tiles, (const int32_t*)workspace, obj_points,
                           out_cap, info);
    else
        hipLaunchKernelGGL(pda::gx_write_kernel<false>, grid, dim3(pda::FS_TILE), 0, (hipStream_t)stream, points, offsets, n_total, c,
                           n_cap, boxes, box_offsets, m_total, centre, obj_offsets, tiles, (const int32_t*)workspace, obj_points,
                           out_cap, info);
    return pda::check_launch("pda_gt_extract_write");
}
