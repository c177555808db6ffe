// spc_sample.hip -- what PV-RCNN++ adds in front of and inside its keypoint encoder (include/pda_train.h):
//   pda_roi_point_filter          sample_points_with_roi (voxel_set_abstraction.py:45-75) and the sector index of sector_fps
//                                 (:88-90) for a whole stacked batch in one launch, without the N x M distance matrix
//   pda_vector_interp_fwd / _bwd  the rows VectorPoolLocalInterpolateModule.forward (pointnet2_modules.py:220-238) assembles
//                                 from the three-NN result: blend, nine relative coordinates, zeros for empty cells
//
// The filter.  One thread per point, one workgroup per 256-point tile of ONE scene, so a workgroup stages the RoIs of one scene
// only.  The counts live on the device: the grid holds divup(n, 256) + b workgroups (a scene adds at most one partial tile)
// and a workgroup past the last tile leaves.  A RoI is four floats in LDS -- centre and half diagonal, the latter taken once
// per RoI and not once per (point, RoI) -- in tiles of 256 RoIs (4 KB); every lane reads the same RoI at the same time, which
// LDS serves as a broadcast.  Per (point, RoI) that is three subtractions, three multiplies, two adds, a sqrt and a compare.
// The interpolation kernels are element-wise over the output (forward) and over the feature part of the gradient (backward):
// both are bound by the rows they move.
#include "pda_common.h"

namespace pda {

constexpr int SPC_TILE = 256;
constexpr int SPC_MAX_B = 1024;

__global__ __launch_bounds__(SPC_TILE) void roi_point_filter_kernel(const float* __restrict__ points,
                                                                    const int* __restrict__ cnt,
                                                                    const float* __restrict__ rois, float radius,
                                                                    float sector_size, uint8_t* __restrict__ mask,
                                                                    int* __restrict__ keys, int64_t n, int b, int m,
                                                                    int roi_stride, int num_sectors) {
    __shared__ float roi[SPC_TILE * 4];
    __shared__ int64_t where[3];                   // scene, its first row, the tile's first row
    if (threadIdx.x == 0) {
        int64_t tiles = 0, row = 0;
        int scene = -1;
        for (int s = 0; s < b; ++s) {
            const int64_t c = max(cnt[s], 0), t = (c + SPC_TILE - 1) / SPC_TILE;
            if ((int64_t)blockIdx.x < tiles + t) {
                scene = s;
                where[1] = row;
                where[2] = row + ((int64_t)blockIdx.x - tiles) * SPC_TILE;
                break;
            }
            tiles += t;
            row += c;
        }
        where[0] = scene;
    }
    __syncthreads();
    const int scene = (int)where[0];
    if (scene < 0) return;                         // uniform: a workgroup past the last tile
    const int64_t end = min(where[1] + max(cnt[scene], 0), n);      // counts that overrun the rows read nothing
    const int64_t p = where[2] + threadIdx.x;
    const bool live = p < end;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) { x = points[p * 3 + 0]; y = points[p * 3 + 1]; z = points[p * 3 + 2]; }
    float best = INFINITY, best_half = 0.f;
    for (int r0 = 0; r0 < m; r0 += SPC_TILE) {
        const int nr = min(SPC_TILE, m - r0);
        __syncthreads();
        if ((int)threadIdx.x < nr) {
            const float* src = rois + ((size_t)scene * m + r0 + threadIdx.x) * roi_stride;
            const float hx = src[3] / 2, hy = src[4] / 2, hz = src[5] / 2;
            roi[threadIdx.x * 4 + 0] = src[0];
            roi[threadIdx.x * 4 + 1] = src[1];
            roi[threadIdx.x * 4 + 2] = src[2];
            roi[threadIdx.x * 4 + 3] = sqrtf((hx * hx + hy * hy) + hz * hz);
        }
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            const float dx = x - roi[r * 4 + 0], dy = y - roi[r * 4 + 1], dz = z - roi[r * 4 + 2];
            const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
            if (d < best) { best = d; best_half = roi[r * 4 + 3]; }          // strict: the lowest index among equals
        }
    }
    if (!live) return;
    const bool keep = best < best_half + radius;
    mask[p] = keep ? 1 : 0;
    if (num_sectors > 0) {
        int sector = num_sectors;
        if (keep) {
            const float angle = atan2f(y, x) + 3.14159265358979323846f;
            sector = (int)fminf(fmaxf(floorf(angle / sector_size), 0.f), (float)num_sectors);
        }
        keys[p] = scene * (num_sectors + 1) + sector;
    }
}

// e = (centre, cell): the three weights of pointnet2_modules.py:220-222 in float32, left to right
__device__ __forceinline__ void interp_weights(const float* __restrict__ dist, int64_t e, float w[3]) {
    const float r0 = 1.0f / (dist[e * 3 + 0] + 1e-8f), r1 = 1.0f / (dist[e * 3 + 1] + 1e-8f), r2 = 1.0f / (dist[e * 3 + 2] + 1e-8f);
    const float norm = fmaxf((r0 + r1) + r2, 1e-8f);
    w[0] = r0 / norm; w[1] = r1 / norm; w[2] = r2 / norm;
}

__device__ __forceinline__ bool interp_rows_ok(const int* __restrict__ idx, int64_t e, int n, int g[3]) {
    g[0] = idx[e * 3 + 0]; g[1] = idx[e * 3 + 1]; g[2] = idx[e * 3 + 2];
    return g[0] >= 0 && g[0] < n && g[1] >= 0 && g[1] < n && g[2] >= 0 && g[2] < n;   // idx[e][0] == -1: an empty cell
}

__global__ __launch_bounds__(256) void vector_interp_fwd_kernel(const float* __restrict__ dist, const int* __restrict__ idx,
                                                                const float* __restrict__ xyz, const float* __restrict__ feat,
                                                                const float* __restrict__ centers, float* __restrict__ out,
                                                                int64_t total, int n, int c) {
    const int width = c + 9;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t e = o / width;
        const int col = (int)(o % width);
        int g[3];
        float v = 0.f;
        if (interp_rows_ok(idx, e, n, g)) {
            if (col < c) {
                float w[3];
                interp_weights(dist, e, w);
                const float p0 = feat[(size_t)g[0] * c + col], p1 = feat[(size_t)g[1] * c + col], p2 = feat[(size_t)g[2] * c + col];
#if PDA_FP_CONTRACT
                v = __builtin_fmaf(w[2], p2, __builtin_fmaf(w[1], p1, w[0] * p0));     // stack_interpolate_kernel's expression
#else
                v = (w[0] * p0 + w[1] * p1) + w[2] * p2;
#endif
            } else {
                const int k = (col - c) / 3, a = (col - c) % 3;
                v = centers[e * 3 + a] - xyz[(size_t)g[k] * 3 + a];
            }
        }
        out[o] = v;
    }
}

__global__ __launch_bounds__(256) void vector_interp_bwd_kernel(const float* __restrict__ grad_out, const float* __restrict__ dist,
                                                                const int* __restrict__ idx, float* __restrict__ grad_feat,
                                                                int64_t total, int n, int c) {
    const int width = c + 9;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t e = o / c;
        const int col = (int)(o % c);
        int g[3];
        if (!interp_rows_ok(idx, e, n, g)) continue;
        float w[3];
        interp_weights(dist, e, w);
        const float go = grad_out[e * width + col];                              // the row stride skips the coordinates
        atomicAdd(grad_feat + (size_t)g[0] * c + col, go * w[0]);
        atomicAdd(grad_feat + (size_t)g[1] * c + col, go * w[1]);
        atomicAdd(grad_feat + (size_t)g[2] * c + col, go * w[2]);
    }
}

static unsigned spc_grid_for(int64_t total) {
    const int64_t blocks = divup64(total, 256);
    return (unsigned)(blocks < 65536 * 16 ? blocks : 65536 * 16);
}

}  // namespace pda

PDA_API int pda_roi_point_filter(const float* points, const int32_t* point_cnt, const float* rois, float radius, uint8_t* mask,
                                 int32_t* keys, int64_t n, int b, int m, int roi_channels, int num_sectors,
                                 pda_stream_t stream) {
    PDA_REQUIRE(n >= 0 && n <= 0x7fffffff && m >= 0 && roi_channels >= 6 && num_sectors >= 0 && num_sectors < 65536,
                "pda_roi_point_filter: bad size n=%lld m=%d roi_channels=%d num_sectors=%d", (long long)n, m, roi_channels,
                num_sectors);
    if (n == 0 || m == 0) return PDA_OK;
    PDA_REQUIRE(b >= 1 && b <= pda::SPC_MAX_B, "pda_roi_point_filter: batch size %d outside [1, %d]", b, pda::SPC_MAX_B);
    PDA_REQUIRE(points && point_cnt && rois && mask && (keys || num_sectors == 0), "pda_roi_point_filter: null pointer");
    const float sector_size = num_sectors > 0 ? (float)(3.14159265358979323846 * 2 / num_sectors) : 1.0f;
    const unsigned grid = (unsigned)(pda::divup64(n, pda::SPC_TILE) + b);
    hipLaunchKernelGGL(pda::roi_point_filter_kernel, dim3(grid), dim3(pda::SPC_TILE), 0, (hipStream_t)stream, points, point_cnt,
                       rois, radius, sector_size, mask, keys, n, b, m, roi_channels, num_sectors);
    return pda::check_launch("pda_roi_point_filter");
}

#define PDA_INTERP_SIZES(what, m, g, n, c)                                                                                    \
    PDA_REQUIRE((m) >= 0 && (g) >= 0 && (n) >= 0 && (c) >= 0 && (int64_t)(m) * (g) <= 0x7fffffff, what ": bad size m=%d g=%d n=%d c=%d", \
                (m), (g), (n), (c))

PDA_API int pda_vector_interp_fwd(const float* dist, const int32_t* idx, const float* support_xyz, const float* support_features,
                                  const float* grid_centers, float* out, int m, int g, int n, int c, pda_stream_t stream) {
    PDA_INTERP_SIZES("pda_vector_interp_fwd", m, g, n, c);
    const int64_t total = (int64_t)m * g * (c + 9);
    if (total == 0) return PDA_OK;
    PDA_REQUIRE(dist && idx && grid_centers && out && (n == 0 || (support_xyz && (support_features || c == 0))),
                "pda_vector_interp_fwd: null pointer");
    hipLaunchKernelGGL(pda::vector_interp_fwd_kernel, dim3(pda::spc_grid_for(total)), dim3(256), 0, (hipStream_t)stream, dist, idx,
                       support_xyz, support_features, grid_centers, out, total, n, c);
    return pda::check_launch("pda_vector_interp_fwd");
}

PDA_API int pda_vector_interp_bwd(const float* grad_out, const float* dist, const int32_t* idx, float* grad_support_features,
                                  int m, int g, int n, int c, pda_stream_t stream) {
    PDA_INTERP_SIZES("pda_vector_interp_bwd", m, g, n, c);
    const int64_t total = (int64_t)m * g * c;
    if (total == 0 || n == 0) return PDA_OK;
    PDA_REQUIRE(grad_out && dist && idx && grad_support_features, "pda_vector_interp_bwd: null pointer");
    hipLaunchKernelGGL(pda::vector_interp_bwd_kernel, dim3(pda::spc_grid_for(total)), dim3(256), 0, (hipStream_t)stream, grad_out,
                       dist, idx, grad_support_features, total, n, c);
    return pda::check_launch("pda_vector_interp_bwd");
}
