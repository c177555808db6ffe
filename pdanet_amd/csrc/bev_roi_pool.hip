// bev_roi_pool.hip -- SECONDHead.roi_grid_pool (second_head.py:53-110) for the whole batch in one launch
// (include/pda_train.h: pda_bev_roi_grid_pool).
//
// The reference loops over the scenes on the host; each turn builds an (R, G, G, 2) grid with affine_grid and samples an
// `expand`ed (R, C, H, W) view of the scene's map with grid_sample.  Here the 4 G^2 (offset, weight) pairs of a RoI serve
// all its channels: a workgroup owns one RoI and a slab of BEV_SLAB channels, computes the pairs once into LDS
// (bev_roi_grid.h, the hostile-row rule lives there), and then walks the slab's BEV_SLAB * G^2 outputs with consecutive
// lanes on consecutive outputs, so the stores are whole lines and each lane gathers four floats from one (h, w) plane.
// Nothing but the output goes to HBM: no grid, no expanded view.  No backward: the reference detaches the features.
#include "pda_common.h"
#include "bev_roi_grid.h"

namespace pda {

constexpr int BEV_SLAB = 64;                       // channels per workgroup
constexpr int BEV_MAX_G = 16;

__global__ __launch_bounds__(256) void bev_roi_grid_pool_kernel(const float* __restrict__ bev, const float* __restrict__ rois,
                                                                float* __restrict__ out, int r, int c, int h, int w, int g,
                                                                float min_x, float min_y, float cell_x, float cell_y) {
    __shared__ int s_off[4][BEV_MAX_G * BEV_MAX_G];
    __shared__ float s_wt[4][BEV_MAX_G * BEV_MAX_G];
    const int tid = threadIdx.x, g2 = g * g;
    const size_t roi = blockIdx.x;                 // scene * r + row
    const size_t scene = roi / (size_t)r;
    if (tid < g2) {
        const float* b = rois + roi * 7;
        float box[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) box[k] = b[k];
        // a heading that is not finite never reaches cosf / sinf; its row reads nothing
        const bool ok = bev_finite_bits(box[6]);
        const float angle = ok ? box[6] : 0.f;
        const BevTheta th = bev_roi_theta(box, cosf(angle), sinf(angle), w, h, min_x, min_y, cell_x, cell_y);
        float ix, iy;
        bev_roi_position(th, tid / g, tid % g, g, w, h, ix, iy);
        BevCorners cr;
        if (!ok) ix = __uint_as_float(0x7fc00000u);
        bev_roi_corners(ix, iy, w, h, cr);
#pragma unroll
        for (int k = 0; k < 4; ++k) { s_off[k][tid] = cr.off[k]; s_wt[k][tid] = cr.wt[k]; }
    }
    __syncthreads();
    const int c0 = blockIdx.y * BEV_SLAB, nc = min(BEV_SLAB, c - c0);
    const size_t plane = (size_t)h * w;
    const float* src = bev + (scene * c + c0) * plane;
    float* dst = out + (roi * c + c0) * g2;
    const int total = nc * g2, dc = 256 / g2, ds = 256 % g2;
    int ch = tid / g2, s = tid % g2;
    for (int e = tid; e < total; e += 256) {
        const float* p = src + (size_t)ch * plane;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int o = s_off[k][s];
            const float v = o >= 0 ? p[o] : 0.f;
            const float t = s_wt[k][s] * v;
            acc = k == 0 ? t : acc + t;            // ((nw + ne) + sw) + se
        }
        dst[e] = acc;
        ch += dc; s += ds;
        if (s >= g2) { s -= g2; ++ch; }
    }
}

}  // namespace pda

PDA_API int pda_bev_roi_grid_pool(const float* bev, const float* rois, float* out, int b, int r, int c, int h, int w, int g,
                                  float min_x, float min_y, float cell_x, float cell_y, pda_stream_t stream) {
    PDA_REQUIRE(b >= 0 && r >= 0 && b <= 65535 && r <= 4096, "pda_bev_roi_grid_pool: bad size batch=%d (0..65535) rois=%d (0..4096)",
                b, r);
    PDA_REQUIRE(g >= 1 && g <= pda::BEV_MAX_G && c >= 1 && c <= 65535 * pda::BEV_SLAB,
                "pda_bev_roi_grid_pool: bad size grid=%d (1..16) channels=%d (1..%d)", g, c, 65535 * pda::BEV_SLAB);
    PDA_REQUIRE(h >= 2 && w >= 2, "pda_bev_roi_grid_pool: map %d x %d: the reference's theta divides by h - 1 and w - 1", h, w);
    PDA_REQUIRE(h <= (1 << 24) && w <= (1 << 24) && (int64_t)h * w <= 0x7fffffff, "pda_bev_roi_grid_pool: map %d x %d too large",
                h, w);
    if (b == 0 || r == 0) return PDA_OK;
    PDA_REQUIRE(bev && rois && out, "pda_bev_roi_grid_pool: null pointer");
    hipLaunchKernelGGL(pda::bev_roi_grid_pool_kernel, dim3((unsigned)(b * r), pda::divup(c, pda::BEV_SLAB)), dim3(256), 0,
                       (hipStream_t)stream, bev, rois, out, r, c, h, w, g, min_x, min_y, cell_x, cell_y);
    return pda::check_launch("pda_bev_roi_grid_pool");
}
