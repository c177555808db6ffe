// stack_pool.hip -- the voxel-query and vector-pool half of the pointnet2_stack operator set
// (include/pda_pointnet2_stack.h): voxel_query_gpu.cu:10-89 and vector_pool_gpu.cu:19-458 of the reference.
// Never reached by PDA-SSD.  voxel_query feeds Voxel R-CNN's RoI-grid pooling (voxel_pool.hip, voxel_pool_modules.py); the
// vector-pool entries are there so that the reference's PV-RCNN++ call sites bind to the same library.
//
// Scene lookup, stream, status codes and pda_last_error() as in stack_ops.hip.  The M x N neighbourhood searches stage
// the scene's points through LDS in 256-point tiles shared by a workgroup of 256 centres.  Instead of the reference's
// per-thread `int temp_idxs[1000]` (4 KB of runtime-indexed private memory per lane: scratch) the neighbour list is
// built by a count pass, a scan over the centres and a fill pass that writes in place; starts therefore do not depend
// on the order in which workgroups run.  vector_pool keeps each tile's hits as a 256-bit mask per centre in LDS: the
// centre's own lane does the sequential bookkeeping (counts, xyz sums, rows of grouped_idxs, nsample), then groups of
// lanes sized to the channels of one cell walk the hits in ascending k and add the contiguous feature rows, so every
// output element is summed in the reference's order (k ascending, then input channel ascending).
#include "pda_common.h"

namespace pda {

constexpr int POOL_MAX_B = 1024;
constexpr int POOL_TILE = 256;
constexpr int POOL_MAX_CANDIDATES = 1000;          // vector_pool_gpu.cu:162,184

__device__ __forceinline__ void pool_prefix(const int* __restrict__ cnt, int b, int* prefix) {
    int acc = 0;
    for (int k = 0; k < b; ++k) { prefix[k] = acc; acc += cnt[k]; }
    prefix[b] = acc;
}
// scene of global index i: the kernels' scan semantics (vector_pool_gpu.cu:140-145): indices past the total stay in
// the last scene
__device__ __forceinline__ int pool_scene(const int* prefix, int b, int i) {
    int bs = 0;
    for (int k = 1; k < b; ++k) bs = (i >= prefix[k]) ? k : bs;
    return bs;
}

// the neighbourhood test of vector_pool_gpu.cu:170-183 / :299-312: ball skips on dist2 > r^2, cube when any |local| > d
__device__ __forceinline__ bool pool_hit(float sx, float sy, float sz, float qx, float qy, float qz, float d, float r2,
                                         int ball) {
    if (ball) return !(sqdist3(sx, sy, sz, qx, qy, qz) > r2);
    const float lx = sx - qx, ly = sy - qy, lz = sz - qz;
    return !(fabsf(lx) > d || fabsf(ly) > d || fabsf(lz) > d);
}

// cell of a hit (vector_pool_gpu.cu:314-318): true divisions, the clamp on the linearised index only
__device__ __forceinline__ int pool_cell(float lx, float ly, float lz, float d, float gsx, float gsy, float gsz, int ngy,
                                         int ngz, int n_grids) {
    const int gx = (int)floorf((lx + d) / gsx), gy = (int)floorf((ly + d) / gsy), gz = (int)floorf((lz + d) / gsz);
    const int cell = gx * ngy * ngz + gy * ngz + gz;
    return min(max(cell, 0), n_grids - 1);
}

// ---- voxel_query -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stack_voxel_query_kernel(int m, int nb, int r1, int r2, int r3, int nsample,
                                                                float radius2, int z_range, int y_range, int x_range,
                                                                const float* __restrict__ new_xyz,
                                                                const float* __restrict__ xyz, int n,
                                                                const int* __restrict__ new_coords,
                                                                const int* __restrict__ point_indices,
                                                                int* __restrict__ idx) {
    const int pt = blockIdx.x * 256 + threadIdx.x;
    if (pt >= m) return;
    const float qx = new_xyz[(size_t)pt * 3 + 0], qy = new_xyz[(size_t)pt * 3 + 1], qz = new_xyz[(size_t)pt * 3 + 2];
    const int bi = new_coords[(size_t)pt * 4 + 0];
    const int64_t cz = new_coords[(size_t)pt * 4 + 1], cy = new_coords[(size_t)pt * 4 + 2], cx = new_coords[(size_t)pt * 4 + 3];
    int* my_idx = idx + (size_t)pt * nsample;
    int cnt = 0;
    if (bi >= 0 && bi < nb) {                      // a batch index outside the grid has no cells
        const int64_t z0 = max(cz - z_range, (int64_t)0), z1 = min(cz + z_range, (int64_t)r1 - 1);
        const int64_t y0 = max(cy - y_range, (int64_t)0), y1 = min(cy + y_range, (int64_t)r2 - 1);
        const int64_t x0 = max(cx - x_range, (int64_t)0), x1 = min(cx + x_range, (int64_t)r3 - 1);
        for (int64_t z = z0; z <= z1 && cnt < nsample; ++z)
            for (int64_t y = y0; y <= y1 && cnt < nsample; ++y) {
                const int* row = point_indices + (((int64_t)bi * r1 + z) * r2 + y) * r3;
                for (int64_t x = x0; x <= x1; ++x) {
                    const int g = row[x];
                    if (g < 0 || g >= n) continue;
                    const float d2 = sqdist3(xyz[(size_t)g * 3 + 0], xyz[(size_t)g * 3 + 1], xyz[(size_t)g * 3 + 2], qx, qy, qz);
                    if (d2 > radius2) continue;
                    if (cnt == 0)
                        for (int l = 0; l < nsample; ++l) my_idx[l] = g;
                    my_idx[cnt] = g;
                    if (++cnt >= nsample) break;   // nothing after the nsample-th hit changes the row
                }
            }
    }
    if (cnt == 0) my_idx[0] = -1;
}

// ---- query_stacked_local_neighbor_idxs: count pass / fill pass ------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(256) void stack_neighbor_kernel(const float* __restrict__ xyz, const int* __restrict__ cnt,
                                                             const float* __restrict__ q_xyz,
                                                             const int* __restrict__ q_cnt, int b, int m, float d,
                                                             int cap, int ball, int* __restrict__ start_len,
                                                             int* __restrict__ out, int64_t max_thresh) {
    __shared__ int qpre[POOL_MAX_B + 1], ppre[POOL_MAX_B + 1];
    __shared__ float tile[POOL_TILE * 3];
    if (threadIdx.x == 0) pool_prefix(q_cnt, b, qpre);
    if (threadIdx.x == 64) pool_prefix(cnt, b, ppre);
    __syncthreads();
    const int pt = blockIdx.x * 256 + threadIdx.x;
    const bool live = pt < m;
    const int first = blockIdx.x * 256, last = min(m, first + 256) - 1;
    const int s_lo = pool_scene(qpre, b, first), s_hi = pool_scene(qpre, b, last);
    const int my_scene = live ? pool_scene(qpre, b, pt) : -1;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) { qx = q_xyz[(size_t)pt * 3 + 0]; qy = q_xyz[(size_t)pt * 3 + 1]; qz = q_xyz[(size_t)pt * 3 + 2]; }
    const float r2 = d * d;
    int found = 0;
    int64_t my_start = 0;
    if (FILL && live) {
        my_start = start_len[(size_t)pt * 2 + 0];
        cap = start_len[(size_t)pt * 2 + 1];       // the count pass' result: the fill pass stops where it stopped
        if (my_start < 0 || my_start >= max_thresh) cap = 0;
    }
    for (int s = s_lo; s <= s_hi; ++s) {
        const int start = ppre[s], n = ppre[s + 1] - ppre[s];
        for (int k0 = 0; k0 < n; k0 += POOL_TILE) {
            const int nk = min(POOL_TILE, n - k0);
            __syncthreads();
            for (int e = threadIdx.x; e < nk * 3; e += 256) tile[e] = xyz[(size_t)(start + k0) * 3 + e];
            __syncthreads();
            if (my_scene != s || found >= cap) continue;
            for (int k = 0; k < nk; ++k) {
                if (!pool_hit(tile[k * 3 + 0], tile[k * 3 + 1], tile[k * 3 + 2], qx, qy, qz, d, r2, ball)) continue;
                if (FILL && my_start + found < max_thresh) out[my_start + found] = start + k0 + k;
                if (++found >= cap) break;
            }
        }
    }
    if (!FILL && live) start_len[(size_t)pt * 2 + 1] = found;
}

// start_len[:, 0] = cumsum[0] + exclusive scan of start_len[:, 1]; cumsum[0] += total.  One workgroup: M is a few
// thousand centres and the pass is a few KB.
__global__ __launch_bounds__(1024) void stack_neighbor_scan_kernel(int* __restrict__ start_len, int* __restrict__ cumsum,
                                                                   int m) {
    __shared__ int wave_sum[16];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = cumsum[0];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = 0; base < m; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const int v = i < m ? start_len[(size_t)i * 2 + 1] : 0;
        int incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int before = carry;
        for (int w = 0; w < wave; ++w) before += wave_sum[w];
        if (i < m) start_len[(size_t)i * 2 + 0] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) cumsum[0] = carry;
}

// ---- query_three_nn_by_stacked_local_idxs -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void stack_three_nn_local_kernel(const float* __restrict__ support_xyz, int n,
                                                                   const float* __restrict__ centers,
                                                                   int* __restrict__ out_idx, float* __restrict__ out_dist2,
                                                                   const int* __restrict__ neighbor_idxs, int64_t n_idxs,
                                                                   const int* __restrict__ start_len, int64_t total,
                                                                   int n_grids) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t pt = e / n_grids;
    const float cx = centers[e * 3 + 0], cy = centers[e * 3 + 1], cz = centers[e * 3 + 2];
    int64_t start = start_len[pt * 2 + 0];
    int64_t len = start_len[pt * 2 + 1];
    if (start < 0 || start >= n_idxs) len = 0;     // a list that was cut, or never written
    len = min(len, n_idxs - start);
    double b1 = 1e40, b2 = 1e40, b3 = 1e40;        // best* are double in the reference
    int i1 = -1, i2 = -1, i3 = -1;
    for (int64_t k = 0; k < len; ++k) {
        const int g = neighbor_idxs[start + k];
        if (g < 0 || g >= n) continue;
        const float d = sqdist3(cx, cy, cz, support_xyz[(size_t)g * 3 + 0], support_xyz[(size_t)g * 3 + 1], support_xyz[(size_t)g * 3 + 2]);
        if (d < b1) { b3 = b2; i3 = i2; b2 = b1; i2 = i1; b1 = d; i1 = g; }
        else if (d < b2) { b3 = b2; i3 = i2; b2 = d; i2 = g; }
        else if (d < b3) { b3 = d; i3 = g; }
    }
    if (i2 == -1) { i2 = i1; b2 = b1; }
    if (i3 == -1) { i3 = i1; b3 = b1; }
    out_dist2[e * 3 + 0] = (float)b1; out_dist2[e * 3 + 1] = (float)b2; out_dist2[e * 3 + 2] = (float)b3;
    out_idx[e * 3 + 0] = i1; out_idx[e * 3 + 1] = i2; out_idx[e * 3 + 2] = i3;
}

// ---- vector_pool ---------------------------------------------------------------------------------------------------
struct PoolArgs {
    const float* xyz; const float* feat; const int* cnt; const float* q_xyz; const int* q_cnt;
    float* new_feat; float* new_lxyz; int* pcnt; int* grouped; int* cum_sum;
    int b, m, c_in, c_out, ce, n_grids, ngy, ngz;
    float d, gsx, gsy, gsz;
    int use_xyz, max_rows, nsample, ball, wlog;
};

template <int POOL>
__global__ __launch_bounds__(256) void stack_vector_pool_kernel(const PoolArgs a) {
    __shared__ int qpre[POOL_MAX_B + 1], ppre[POOL_MAX_B + 1];
    __shared__ float tile[POOL_TILE * 3], ctr[256 * 3];
    __shared__ uint32_t mask[POOL_TILE / 32][256];
    __shared__ uint32_t any_hit[256];
    if (threadIdx.x == 0) pool_prefix(a.q_cnt, a.b, qpre);
    if (threadIdx.x == 64) pool_prefix(a.cnt, a.b, ppre);
    const int tid = threadIdx.x;
    const int pt = blockIdx.x * 256 + tid;
    const bool live = pt < a.m;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) { qx = a.q_xyz[(size_t)pt * 3 + 0]; qy = a.q_xyz[(size_t)pt * 3 + 1]; qz = a.q_xyz[(size_t)pt * 3 + 2]; }
    ctr[tid * 3 + 0] = qx; ctr[tid * 3 + 1] = qy; ctr[tid * 3 + 2] = qz;
    __syncthreads();
    const int first = blockIdx.x * 256, last = min(a.m, first + 256) - 1;
    const int s_lo = pool_scene(qpre, a.b, first), s_hi = pool_scene(qpre, a.b, last);
    const int my_scene = live ? pool_scene(qpre, a.b, pt) : -1;
    const float r2 = a.d * a.d;
    int* my_cnt = a.pcnt + (size_t)pt * a.n_grids;
    float* my_lxyz = a.new_lxyz + (size_t)pt * a.n_grids * 3;
    int sample_cnt = 0;
    bool done = false;
    // feature pass: groups of 2^wlog lanes, one centre per group and round
    const int lane = lane_id(), wave = wave_id();
    const int gw = 1 << a.wlog, n_groups = 64 >> a.wlog, sub = lane >> a.wlog, j0 = lane & (gw - 1);

    for (int s = s_lo; s <= s_hi; ++s) {
        const int start = ppre[s], n = ppre[s + 1] - ppre[s];
        for (int k0 = 0; k0 < n; k0 += POOL_TILE) {
            const int nk = min(POOL_TILE, n - k0);
            __syncthreads();                       // the feature pass of the tile before is done with tile and mask
            for (int e = tid; e < nk * 3; e += 256) tile[e] = a.xyz[(size_t)(start + k0) * 3 + e];
            __syncthreads();
            uint32_t w[POOL_TILE / 32];
#pragma unroll
            for (int wi = 0; wi < POOL_TILE / 32; ++wi) w[wi] = 0;
            if (my_scene == s && !done) {
                int total = 0;
#pragma unroll
                for (int wi = 0; wi < POOL_TILE / 32; ++wi) {
                    uint32_t word = 0;
                    if (wi * 32 < nk) {
                        for (int bi = 0; bi < 32; ++bi) {
                            const int k = wi * 32 + bi;
                            const bool hit = pool_hit(tile[k * 3 + 0], tile[k * 3 + 1], tile[k * 3 + 2], qx, qy, qz, a.d, r2, a.ball);
                            word |= (hit && k < nk) ? (1u << bi) : 0u;
                        }
                    }
                    w[wi] = word;
                    total += __popc(word);
                }
                if (POOL == 0) {
                    // one reservation per centre and tile instead of one atomic per hit; with nsample > 0 only the rows
                    // the centre still takes are reserved, so the returned total is what a call that fits needs
                    const int take = a.nsample > 0 ? min(total, a.nsample - sample_cnt) : total;
                    const int base = take > 0 ? atomicAdd(a.cum_sum, take) : 0;
                    int seen = 0;
#pragma unroll
                    for (int wi = 0; wi < POOL_TILE / 32; ++wi) {
                        uint32_t word = w[wi], keep = 0;
                        while (word && seen < take) {
                            const int bi = __ffs(word) - 1;
                            word &= word - 1;
                            keep |= 1u << bi;
                            const int k = wi * 32 + bi;
                            const float lx = tile[k * 3 + 0] - qx, ly = tile[k * 3 + 1] - qy, lz = tile[k * 3 + 2] - qz;
                            const int cell = pool_cell(lx, ly, lz, a.d, a.gsx, a.gsy, a.gsz, a.ngy, a.ngz, a.n_grids);
                            my_cnt[cell]++;
                            if (a.use_xyz) { my_lxyz[cell * 3 + 0] += lx; my_lxyz[cell * 3 + 1] += ly; my_lxyz[cell * 3 + 2] += lz; }
                            const int row = base + seen;
                            if (row >= 0 && row < a.max_rows) {
                                a.grouped[(size_t)row * 3 + 0] = start + k0 + k;
                                a.grouped[(size_t)row * 3 + 1] = pt;
                                a.grouped[(size_t)row * 3 + 2] = cell;
                            }
                            ++seen;
                        }
                        w[wi] = keep;
                    }
                    sample_cnt += take;
                    done = a.nsample > 0 && sample_cnt >= a.nsample;
                } else {
#pragma unroll
                    for (int wi = 0; wi < POOL_TILE / 32; ++wi) {
                        uint32_t word = w[wi], keep = 0;
                        while (word && !done) {
                            const int bi = __ffs(word) - 1;
                            word &= word - 1;
                            const int k = wi * 32 + bi;
                            const float lx = tile[k * 3 + 0] - qx, ly = tile[k * 3 + 1] - qy, lz = tile[k * 3 + 2] - qz;
                            const int cell = pool_cell(lx, ly, lz, a.d, a.gsx, a.gsy, a.gsz, a.ngy, a.ngz, a.n_grids);
                            if (my_cnt[cell] != 0) continue;                 // only the first point of a cell
                            my_cnt[cell]++;
                            keep |= 1u << bi;
                            if (a.use_xyz) { my_lxyz[cell * 3 + 0] = lx; my_lxyz[cell * 3 + 1] = ly; my_lxyz[cell * 3 + 2] = lz; }
                            const int row = atomicAdd(a.cum_sum, 1);
                            if (row < 0 || row >= a.max_rows) continue;      // keeps counting what a call that fits needs
                            a.grouped[(size_t)row * 3 + 0] = start + k0 + k;
                            a.grouped[(size_t)row * 3 + 1] = pt;
                            a.grouped[(size_t)row * 3 + 2] = cell;
                            ++sample_cnt;
                            done = (a.nsample > 0 && sample_cnt >= a.nsample) || sample_cnt >= a.n_grids;
                        }
                        w[wi] = keep;
                    }
                }
            }
            uint32_t any = 0;
#pragma unroll
            for (int wi = 0; wi < POOL_TILE / 32; ++wi) { mask[wi][tid] = w[wi]; any |= w[wi]; }
            any_hit[tid] = any;
            __syncthreads();
            // feature pass: lane j0 of a group owns the outputs j0, j0 + gw, ... of every cell of the group's centre
            for (int r = 0; r < gw; ++r) {
                const int cl = wave * 64 + r * n_groups + sub;
                if (!any_hit[cl]) continue;
                const float cx = ctr[cl * 3 + 0], cy = ctr[cl * 3 + 1], cz = ctr[cl * 3 + 2];
                float* orow0 = a.new_feat + (size_t)(first + cl) * a.c_out;
                for (int wi = 0; wi < POOL_TILE / 32; ++wi) {
                    uint32_t word = mask[wi][cl];
                    while (word) {
                        const int bi = __ffs(word) - 1;
                        word &= word - 1;
                        const int k = wi * 32 + bi;
                        const float lx = tile[k * 3 + 0] - cx, ly = tile[k * 3 + 1] - cy, lz = tile[k * 3 + 2] - cz;
                        const int cell = pool_cell(lx, ly, lz, a.d, a.gsx, a.gsy, a.gsz, a.ngy, a.ngz, a.n_grids);
                        const float* frow = a.feat + (size_t)(start + k0 + k) * a.c_in;
                        float* orow = orow0 + (size_t)cell * a.ce;
                        for (int j = j0; j < a.ce; j += gw) {
                            float acc = POOL == 0 ? orow[j] : 0.f;
                            for (int i = j; i < a.c_in; i += a.ce) acc = POOL == 0 ? acc + frow[i] : frow[i];
                            if (j < a.c_in) orow[j] = acc;
                        }
                    }
                }
            }
        }
    }
}

// grad_support[k, c] += grad_new[centre, cell * ce + c % ce] / max(cnt, 1) per grouped_idxs row and input channel
__global__ __launch_bounds__(256) void stack_vector_pool_grad_kernel(const float* __restrict__ grad_new,
                                                                     const int* __restrict__ pcnt,
                                                                     const int* __restrict__ grouped,
                                                                     float* __restrict__ grad_support, int n, int m,
                                                                     int c_out, int c_in, int ce, int n_grids,
                                                                     int64_t total) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / c_in;
        const int c = (int)(e % c_in);
        const int k = grouped[row * 3 + 0], pt = grouped[row * 3 + 1], cell = grouped[row * 3 + 2];
        if (k < 0 || k >= n || pt < 0 || pt >= m || cell < 0 || cell >= n_grids) continue;
        const float cnt = fmaxf((float)pcnt[(size_t)pt * n_grids + cell], 1.0f);
        atomicAdd(grad_support + (size_t)k * c_in + c, grad_new[(size_t)pt * c_out + (size_t)cell * ce + c % ce] / cnt);
    }
}

}  // namespace pda

#define PDA_POOL_B(b, what) PDA_REQUIRE((b) >= 1 && (b) <= pda::POOL_MAX_B, what ": batch size %d outside [1, %d]", (b), pda::POOL_MAX_B)

PDA_API int pda_stack_voxel_query(const float* new_xyz, const float* xyz, const int32_t* new_coords,
                                  const int32_t* point_indices, int32_t* idx, int b, int n, int m, int r1, int r2, int r3,
                                  int nsample, float radius, int z_range, int y_range, int x_range, pda_stream_t stream) {
    PDA_REQUIRE(m >= 0 && n >= 0 && nsample >= 1 && r1 >= 1 && r2 >= 1 && r3 >= 1 && z_range >= 0 && y_range >= 0 && x_range >= 0,
                "pda_stack_voxel_query: bad size m=%d n=%d nsample=%d grid=(%d,%d,%d) range=(%d,%d,%d)", m, n, nsample, r1, r2,
                r3, z_range, y_range, x_range);
    if (m == 0) return PDA_OK;
    PDA_REQUIRE(b >= 1, "pda_stack_voxel_query: batch size %d", b);
    PDA_REQUIRE(new_xyz && xyz && new_coords && point_indices && idx, "pda_stack_voxel_query: null pointer");
    hipLaunchKernelGGL(pda::stack_voxel_query_kernel, dim3(pda::divup(m, 256)), dim3(256), 0, (hipStream_t)stream, m, b, r1, r2,
                       r3, nsample, radius * radius, z_range, y_range, x_range, new_xyz, xyz, n, new_coords, point_indices, idx);
    return pda::check_launch("pda_stack_voxel_query");
}

PDA_API int pda_stack_query_local_neighbor_idxs(const float* support_xyz, const int32_t* xyz_batch_cnt, const float* new_xyz,
                                                const int32_t* new_xyz_batch_cnt, int32_t* stack_neighbor_idxs,
                                                int32_t* start_len, int32_t* cumsum, int avg_length_of_neighbor_idxs,
                                                float max_neighbour_distance, int b, int m, int nsample, int neighbor_type,
                                                pda_stream_t stream) {
    PDA_REQUIRE(m >= 0 && avg_length_of_neighbor_idxs >= 0, "pda_stack_query_local_neighbor_idxs: bad size m=%d avg_length=%d", m,
                avg_length_of_neighbor_idxs);
    if (m == 0) return PDA_OK;
    PDA_POOL_B(b, "pda_stack_query_local_neighbor_idxs");
    PDA_REQUIRE(support_xyz && xyz_batch_cnt && new_xyz && new_xyz_batch_cnt && stack_neighbor_idxs && start_len && cumsum,
                "pda_stack_query_local_neighbor_idxs: null pointer");
    const int cap = nsample > 0 && nsample < pda::POOL_MAX_CANDIDATES ? nsample : pda::POOL_MAX_CANDIDATES;
    const int64_t max_thresh = (int64_t)avg_length_of_neighbor_idxs * m;
    const int ball = neighbor_type == 1;
    const dim3 grid(pda::divup(m, 256));
    hipLaunchKernelGGL(pda::stack_neighbor_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, support_xyz, xyz_batch_cnt,
                       new_xyz, new_xyz_batch_cnt, b, m, max_neighbour_distance, cap, ball, start_len, stack_neighbor_idxs,
                       max_thresh);
    hipLaunchKernelGGL(pda::stack_neighbor_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, start_len, cumsum, m);
    hipLaunchKernelGGL(pda::stack_neighbor_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, support_xyz, xyz_batch_cnt,
                       new_xyz, new_xyz_batch_cnt, b, m, max_neighbour_distance, cap, ball, start_len, stack_neighbor_idxs,
                       max_thresh);
    return pda::check_launch("pda_stack_query_local_neighbor_idxs");
}

PDA_API int pda_stack_three_nn_by_local_idxs(const float* support_xyz, const float* new_xyz_grid_centers,
                                             int32_t* new_xyz_grid_idxs, float* new_xyz_grid_dist2,
                                             const int32_t* stack_neighbor_idxs, const int32_t* start_len, int n,
                                             int64_t num_neighbor_idxs, int m, int num_total_grids, pda_stream_t stream) {
    PDA_REQUIRE(m >= 0 && n >= 0 && num_total_grids >= 0 && num_neighbor_idxs >= 0,
                "pda_stack_three_nn_by_local_idxs: bad size m=%d n=%d num_total_grids=%d", m, n, num_total_grids);
    const int64_t total = (int64_t)m * num_total_grids;
    if (total == 0) return PDA_OK;
    PDA_REQUIRE(pda::divup64(total, 256) <= 0x7fffffff, "pda_stack_three_nn_by_local_idxs: m * num_total_grids too large");
    PDA_REQUIRE(new_xyz_grid_centers && new_xyz_grid_idxs && new_xyz_grid_dist2 && start_len &&
                    (num_neighbor_idxs == 0 || (stack_neighbor_idxs && support_xyz)),
                "pda_stack_three_nn_by_local_idxs: null pointer");
    hipLaunchKernelGGL(pda::stack_three_nn_local_kernel, dim3((unsigned)pda::divup64(total, 256)), dim3(256), 0,
                       (hipStream_t)stream, support_xyz, n, new_xyz_grid_centers, new_xyz_grid_idxs, new_xyz_grid_dist2,
                       stack_neighbor_idxs, num_neighbor_idxs, start_len, total, num_total_grids);
    return pda::check_launch("pda_stack_three_nn_by_local_idxs");
}

PDA_API int pda_stack_vector_pool(const float* support_xyz, const float* support_features, const int32_t* xyz_batch_cnt,
                                  const float* new_xyz, const int32_t* new_xyz_batch_cnt, float* new_features,
                                  float* new_local_xyz, int32_t* point_cnt_of_grid, int32_t* grouped_idxs,
                                  int32_t* num_cum_sum, int b, int m, int c_in, int c_out, int num_total_grids,
                                  int num_grid_x, int num_grid_y, int num_grid_z, float max_neighbour_distance, int use_xyz,
                                  int num_max_sum_points, int nsample, int neighbor_type, int pooling_type,
                                  pda_stream_t stream) {
    PDA_REQUIRE(m >= 0 && c_in >= 1 && num_total_grids >= 1 && c_out >= num_total_grids && num_grid_x >= 1 && num_grid_y >= 1 &&
                    num_grid_z >= 1 && num_max_sum_points >= 0,
                "pda_stack_vector_pool: bad size m=%d c_in=%d c_out=%d num_total_grids=%d grid=(%d,%d,%d) num_max_sum_points=%d", m,
                c_in, c_out, num_total_grids, num_grid_x, num_grid_y, num_grid_z, num_max_sum_points);
    PDA_REQUIRE(pooling_type == 0 || pooling_type == 1, "pda_stack_vector_pool: pooling_type %d is neither 0 (sum) nor 1 (first)",
                pooling_type);
    if (m == 0) return PDA_OK;
    PDA_POOL_B(b, "pda_stack_vector_pool");
    PDA_REQUIRE(support_xyz && support_features && xyz_batch_cnt && new_xyz && new_xyz_batch_cnt && new_features &&
                    new_local_xyz && point_cnt_of_grid && (grouped_idxs || num_max_sum_points == 0) && num_cum_sum,
                "pda_stack_vector_pool: null pointer");
    pda::PoolArgs a;
    a.xyz = support_xyz; a.feat = support_features; a.cnt = xyz_batch_cnt; a.q_xyz = new_xyz; a.q_cnt = new_xyz_batch_cnt;
    a.new_feat = new_features; a.new_lxyz = new_local_xyz; a.pcnt = point_cnt_of_grid; a.grouped = grouped_idxs;
    a.cum_sum = num_cum_sum;
    a.b = b; a.m = m; a.c_in = c_in; a.c_out = c_out; a.ce = c_out / num_total_grids; a.n_grids = num_total_grids;
    a.ngy = num_grid_y; a.ngz = num_grid_z;
    a.d = max_neighbour_distance;
    a.gsx = max_neighbour_distance * 2 / num_grid_x;
    a.gsy = max_neighbour_distance * 2 / num_grid_y;
    a.gsz = max_neighbour_distance * 2 / num_grid_z;
    a.use_xyz = use_xyz != 0; a.max_rows = num_max_sum_points; a.nsample = nsample; a.ball = neighbor_type == 1;
    a.wlog = 0;
    while (a.wlog < 6 && (1 << a.wlog) < a.ce) ++a.wlog;
    if (hipMemsetAsync(num_cum_sum, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess)
        return pda::check_launch("pda_stack_vector_pool");
    if (pooling_type == 0)
        hipLaunchKernelGGL(pda::stack_vector_pool_kernel<0>, dim3(pda::divup(m, 256)), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(pda::stack_vector_pool_kernel<1>, dim3(pda::divup(m, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return pda::check_launch("pda_stack_vector_pool");
}

PDA_API int pda_stack_vector_pool_grad(const float* grad_new_features, const int32_t* point_cnt_of_grid,
                                       const int32_t* grouped_idxs, float* grad_support_features, int n, int m, int c_out,
                                       int c_in, int num_total_grids, int num_max_sum_points, pda_stream_t stream) {
    PDA_REQUIRE(n >= 0 && m >= 0 && c_in >= 0 && num_max_sum_points >= 0 && num_total_grids >= 1 && c_out >= num_total_grids,
                "pda_stack_vector_pool_grad: bad size n=%d m=%d c_in=%d c_out=%d num_total_grids=%d num_max_sum_points=%d", n, m,
                c_in, c_out, num_total_grids, num_max_sum_points);
    const int64_t total = (int64_t)num_max_sum_points * c_in;
    if (total == 0 || m == 0 || n == 0) return PDA_OK;
    PDA_REQUIRE(grad_new_features && point_cnt_of_grid && grouped_idxs && grad_support_features,
                "pda_stack_vector_pool_grad: null pointer");
    const int64_t blocks = pda::divup64(total, 256);
    hipLaunchKernelGGL(pda::stack_vector_pool_grad_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                       (hipStream_t)stream, grad_new_features, point_cnt_of_grid, grouped_idxs, grad_support_features, n, m,
                       c_out, c_in, c_out / num_total_grids, num_total_grids, total);
    return pda::check_launch("pda_stack_vector_pool_grad");
}
