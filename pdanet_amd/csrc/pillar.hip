// pillar.hip -- the two pillar operators the pillar detectors share, neither of them a head: PointPillarScatter
// (backbones_2d/map_to_bev/pointpillar_scatter.py) and the PFN input rows of the hard-voxel PillarVFE
// (backbones_3d/vfe/pillar_vfe.py).
//
// Reference: the scatter loops over scenes behind a .item(); PillarVFE builds its rows in about a dozen element-wise passes.
//
// Here: pillar_scatter_kernel, a pillar-by-channel tile transposed through LDS (rows read whole, planes written with the
// pillar on the lane axis), and pillar_features_kernel, one wave per voxel; one launch each.  No atomics.
#include "pda_common.h"

#include <math.h>

namespace pda {
namespace {

// ---- PointPillarScatter ------------------------------------------------------------------------------------------------------
constexpr int PS_TILE = 64;      // pillars and channels of one LDS tile
constexpr int PS_THREADS = 256;

// BWD == false: out[b, c, cell] = feats[p, c]; BWD == true: feats[p, c] = out[b, c, cell] (0 for a skipped row).  `planes` is
// (B, C, ny * nx).  A row is skipped when its batch index is outside [0, B), its cell c1 + c2 * nx + c3 outside the grid, or
// (padded form) its index is not below *count.
template <bool BWD>
__global__ __launch_bounds__(PS_THREADS) void pillar_scatter_kernel(
        float* __restrict__ feats, const int32_t* __restrict__ coords, const int32_t* __restrict__ count, long long n, int C,
        int B, long long cells, int nx, float* __restrict__ planes) {
    __shared__ float tile[PS_TILE][PS_TILE + 1];
    __shared__ long long dest[PS_TILE];
    const long long p0 = (long long)blockIdx.x * PS_TILE;
    const long long live = count ? min((long long)max(count[0], 0), n) : n;
    if (threadIdx.x < PS_TILE) {
        const long long p = p0 + threadIdx.x;
        long long d = -1;
        if (p < live) {
            const int32_t* c = coords + p * 4;
            const long long cell = (long long)c[1] + (long long)c[2] * nx + (long long)c[3];
            if (c[0] >= 0 && c[0] < B && cell >= 0 && cell < cells) d = (long long)c[0] * C * cells + cell;
        }
        dest[threadIdx.x] = d;
    }
    __syncthreads();
    for (int c0 = 0; c0 < C; c0 += PS_TILE) {
        if (!BWD) {
            for (int e = threadIdx.x; e < PS_TILE * PS_TILE; e += PS_THREADS) {
                const int p = e / PS_TILE, c = e % PS_TILE;      // the channel on the lane axis: a row is read whole
                if (p0 + p < n && c0 + c < C && dest[p] >= 0) tile[p][c] = feats[(p0 + p) * C + c0 + c];
            }
            __syncthreads();
            for (int e = threadIdx.x; e < PS_TILE * PS_TILE; e += PS_THREADS) {
                const int c = e / PS_TILE, p = e % PS_TILE;      // the pillar on the lane axis: neighbouring cells
                if (c0 + c < C && dest[p] >= 0) planes[dest[p] + (long long)(c0 + c) * cells] = tile[p][c];
            }
        } else {
            for (int e = threadIdx.x; e < PS_TILE * PS_TILE; e += PS_THREADS) {
                const int c = e / PS_TILE, p = e % PS_TILE;
                if (c0 + c < C) tile[p][c] = dest[p] >= 0 ? planes[dest[p] + (long long)(c0 + c) * cells] : 0.f;
            }
            __syncthreads();
            for (int e = threadIdx.x; e < PS_TILE * PS_TILE; e += PS_THREADS) {
                const int p = e / PS_TILE, c = e % PS_TILE;
                if (p0 + p < n && c0 + c < C) feats[(p0 + p) * C + c0 + c] = tile[p][c];
            }
        }
        __syncthreads();
    }
}

// ---- PillarVFE's PFN input rows ------------------------------------------------------------------------------------------------
struct PillarFeatCfg {
    long long V;
    int P, C, absolute_xyz, with_distance, c_out;
    float vs[3], off[3];      // float32(voxel size), float32(voxel / 2 + range_lo), x y z
};

// One wave per voxel.  The mean is the sum over all P rows IN ROW ORDER (lanes 0..2, one coordinate each) divided by
// num_points; rows from num_points on are written as zeros.
__global__ __launch_bounds__(256) void pillar_features_kernel(const float* __restrict__ voxels,
                                                              const int32_t* __restrict__ num_points,
                                                              const int32_t* __restrict__ coords, PillarFeatCfg g,
                                                              float* __restrict__ out) {
    const long long v = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= g.V) return;      // wave-uniform
    const int lane = (int)(threadIdx.x & 63);
    const int np = num_points[v];
    const float* vox = voxels + (size_t)v * g.P * g.C;
    float sum = 0.f;
    if (lane < 3)
        for (int p = 0; p < g.P; ++p) sum += vox[(size_t)p * g.C + lane];
    const float mean = sum / (float)np;
    const float mx = __shfl(mean, 0), my = __shfl(mean, 1), mz = __shfl(mean, 2);
    const int32_t* c = coords + (size_t)v * 4;
    const float cx = (float)c[3] * g.vs[0] + g.off[0];
    const float cy = (float)c[2] * g.vs[1] + g.off[1];
    const float cz = (float)c[1] * g.vs[2] + g.off[2];
    const int first = g.absolute_xyz ? 0 : 3;
    for (int p = lane; p < g.P; p += 64) {
        const float* row = vox + (size_t)p * g.C;
        float* o = out + ((size_t)v * g.P + p) * g.c_out;
        if (p >= np) {
            for (int k = 0; k < g.c_out; ++k) o[k] = 0.f;
            continue;
        }
        const float x = row[0], y = row[1], z = row[2];
        int k = 0;
        for (int q = first; q < g.C; ++q) o[k++] = row[q];
        o[k++] = x - mx;
        o[k++] = y - my;
        o[k++] = z - mz;
        o[k++] = x - cx;
        o[k++] = y - cy;
        o[k++] = z - cz;
        if (g.with_distance) o[k++] = sqrtf((x * x + y * y) + z * z);
    }
}

}  // namespace
}  // namespace pda

// ---- C entry points ------------------------------------------------------------------------------------------------------------
static int pillar_scatter_check(const char* what, int64_t n, int c, int b, int ny, int nx) {
    PDA_REQUIRE(n >= 0 && c >= 0 && b >= 0 && ny >= 0 && nx >= 0, "%s: n=%lld c=%d b=%d ny=%d nx=%d", what, (long long)n, c, b,
                ny, nx);
    PDA_REQUIRE(n <= (int64_t)INT32_MAX * pda::PS_TILE, "%s: n=%lld too large", what, (long long)n);
    return PDA_OK;
}

PDA_API int pda_pillar_scatter_fwd(const float* features, const int32_t* coords, const int32_t* count, int64_t n, int c, int b,
                                   int ny, int nx, float* out, pda_stream_t stream) {
    if (int st = pillar_scatter_check("pda_pillar_scatter_fwd", n, c, b, ny, nx)) return st;
    if (n == 0 || c == 0 || b == 0 || ny == 0 || nx == 0) return PDA_OK;
    PDA_REQUIRE(features && coords && out, "pda_pillar_scatter_fwd: null pointer");
    hipLaunchKernelGGL(pda::pillar_scatter_kernel<false>, dim3((unsigned)pda::divup64(n, pda::PS_TILE)), dim3(pda::PS_THREADS),
                       0, (hipStream_t)stream, const_cast<float*>(features), coords, count, (long long)n, c, b,
                       (long long)ny * nx, nx, out);
    return pda::check_launch("pda_pillar_scatter_fwd");
}

PDA_API int pda_pillar_scatter_bwd(const float* grad_out, const int32_t* coords, const int32_t* count, int64_t n, int c, int b,
                                   int ny, int nx, float* grad_features, pda_stream_t stream) {
    if (int st = pillar_scatter_check("pda_pillar_scatter_bwd", n, c, b, ny, nx)) return st;
    if (n == 0 || c == 0) return PDA_OK;
    PDA_REQUIRE(b > 0 && ny > 0 && nx > 0, "pda_pillar_scatter_bwd: empty grid with n=%lld rows", (long long)n);
    PDA_REQUIRE(grad_out && coords && grad_features, "pda_pillar_scatter_bwd: null pointer");
    hipLaunchKernelGGL(pda::pillar_scatter_kernel<true>, dim3((unsigned)pda::divup64(n, pda::PS_TILE)), dim3(pda::PS_THREADS),
                       0, (hipStream_t)stream, grad_features, coords, count, (long long)n, c, b, (long long)ny * nx, nx,
                       const_cast<float*>(grad_out));
    return pda::check_launch("pda_pillar_scatter_bwd");
}

PDA_API int pda_pillar_features(const float* voxels, const int32_t* voxel_num_points, const int32_t* voxel_coords, int64_t v,
                                int p, int c, const float* voxel_size3, const float* offset3, int absolute_xyz,
                                int with_distance, float* out, pda_stream_t stream) {
    PDA_REQUIRE(v >= 0 && p >= 0 && v <= (int64_t)INT32_MAX, "pda_pillar_features: v=%lld p=%d", (long long)v, p);
    PDA_REQUIRE(c >= 3 && c <= 64, "pda_pillar_features: c=%d outside 3..64", c);
    if (v == 0 || p == 0) return PDA_OK;
    PDA_REQUIRE(voxels && voxel_num_points && voxel_coords && voxel_size3 && offset3 && out, "pda_pillar_features: null pointer");
    pda::PillarFeatCfg g{};
    g.V = v;
    g.P = p;
    g.C = c;
    g.absolute_xyz = absolute_xyz ? 1 : 0;
    g.with_distance = with_distance ? 1 : 0;
    g.c_out = (absolute_xyz ? c : c - 3) + 6 + (with_distance ? 1 : 0);
    for (int i = 0; i < 3; ++i) {
        g.vs[i] = voxel_size3[i];
        g.off[i] = offset3[i];
    }
    hipLaunchKernelGGL(pda::pillar_features_kernel, dim3((unsigned)pda::divup64(v, 4)), dim3(256), 0, (hipStream_t)stream, voxels,
                       voxel_num_points, voxel_coords, g, out);
    return pda::check_launch("pda_pillar_features");
}
