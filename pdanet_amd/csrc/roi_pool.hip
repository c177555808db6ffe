// roi_pool.hip -- the RoI pooling operators of the two-stage heads (include/pda_train.h): roiaware_pool3d forward and
// backward (roiaware_pool3d_kernel.cu:39-310), roipoint_pool3d forward (roipoint_pool3d_kernel.cu:38-165) and the
// boxes x points mask of points_in_boxes_cpu (roiaware_pool3d.cpp:128-168), and that mask's row sums for a whole batch without
// the mask (SECONDNetIoU's num_pts_iou_cls score), and PointRCNNHead's whole input stage in one launch (the pooling with the
// canonical transformation, the score and depth columns and the zeroing of empty RoIs).  Never reached by PDA-SSD; built so
// that the reference's Part-A2, PointRCNN and SECOND-IoU heads bind to the same library.
//
// The reference writes a boxes x points int mask to HBM, then lets ONE thread per box walk the whole scene.  Here a
// workgroup owns a box and walks the scene in ascending 256-point tiles: every lane tests one point (box_rec.h, the
// trigonometry done once), the tile's hits are compacted in point order with ballots and a prefix over the four waves,
// and every hit finds its slot as (points its voxel already holds) + (earlier hits of the same voxel in this tile), so
// slots 1..count hold the first K-1 points of a voxel in ascending point index whatever order the lanes run in.  No
// mask, no device allocation, no atomics in the forward.  Voxel counters live in LDS when the grid has at most
// ROI_LDS_VOX voxels and in slot 0 of the output otherwise.  Pooling reads 64 counters per wave, keeps the non-empty
// voxels and puts the channel on the lane axis, so feature rows and output rows are read and written whole.
#include "pda_common.h"
#include "box_rec.h"
#include "roi_pool_core.h"

namespace pda {

constexpr int ROIPOINT_MAX_S = 15360;              // 60 KB of sampled indices

// ---- roiaware_pool3d: collect (the walk: roi_pool_core.h) ------------------------------------------------------------------
template <bool LDS_CNT>
__global__ __launch_bounds__(256) void roiaware_collect_kernel(const float* __restrict__ rois, const float* __restrict__ pts,
                                                               int* __restrict__ pts_idx, int pts_num, int out_x, int out_y,
                                                               int out_z, int k_slots) {
    __shared__ int cnt[LDS_CNT ? ROI_LDS_VOX : 1];
    __shared__ int hit_vox[ROI_TILE];
    __shared__ int wave_cnt[2][ROI_TILE / 64];
    int* mine = pts_idx + (size_t)blockIdx.x * (out_x * out_y * out_z) * k_slots;
    roi_collect_walk<LDS_CNT, false>(rois + (size_t)blockIdx.x * 7, pts, 3, 0, pts_num, mine, out_x, out_y, out_z, k_slots, cnt,
                                     hit_vox, wave_cnt);
}

// ---- roiaware_pool3d: pool -----------------------------------------------------------------------------------------------
// A wave takes 64 consecutive voxels of one box: it reads their counters, compacts the non-empty ones, and groups of
// 2^wlog lanes (the channels of one voxel) pool them.  Shared by the forward (POOL 0 max, 1 avg) and the avg backward (2).
template <int MODE>
__global__ __launch_bounds__(256) void roiaware_pool_kernel(const float* __restrict__ feat, const int* __restrict__ pts_idx,
                                                            float* __restrict__ pooled, int* __restrict__ argmax,
                                                            const float* __restrict__ grad_out, float* __restrict__ grad_in,
                                                            int pts_num, int channels, int n_vox, int k_slots, int wlog) {
    __shared__ int s_cnt[ROI_TILE / 64][64];
    __shared__ int s_list[ROI_TILE / 64][64];
    const int lane = lane_id(), wave = wave_id();
    const int v_base = blockIdx.y * ROI_TILE + wave * 64;
    const size_t box_vox = (size_t)blockIdx.x * n_vox;
    const int v = v_base + lane;
    int c = v < n_vox ? pts_idx[(box_vox + v) * k_slots] : 0;
    c = roi_slot_count(c, k_slots);
    s_cnt[wave][lane] = c;
    const uint64_t mask = __ballot(c > 0);
    const int nnz = __popcll(mask);
    if (c > 0) s_list[wave][__popcll(mask & lanes_below())] = lane;
    __syncthreads();
    const int nv = min(64, n_vox - v_base);        // <= 0 for a wave past the grid
    if (MODE == 0 && nnz < nv) {                   // empty voxels: argmax -1, pooled_features untouched
        int* arow = argmax + (box_vox + v_base) * channels;
        for (int i = lane; i < nv * channels; i += 64)
            if (s_cnt[wave][i / channels] == 0) arow[i] = -1;
    }
    const int gw = 1 << wlog, n_groups = 64 >> wlog, sub = lane >> wlog, j0 = lane & (gw - 1);
    for (int e0 = 0; e0 < nnz; e0 += n_groups) {
        const int e = e0 + sub;
        if (e >= nnz) continue;
        const int lv = s_list[wave][e], n = s_cnt[wave][lv];
        const size_t vox = box_vox + v_base + lv;
        const int* idx = pts_idx + vox * k_slots;
        for (int ch = j0; ch < channels; ch += gw) {
            if (MODE == 0) {
                uint32_t best_bits;
                const int arg = roi_slot_max(feat, idx, n, pts_num, channels, ch, best_bits);
                if (arg != -1) pooled[vox * channels + ch] = __uint_as_float(best_bits);
                argmax[vox * channels + ch] = arg;
            } else if (MODE == 1) {
                const float sum = roi_slot_sum(idx, n, pts_num, [&](int p) { return feat[(size_t)p * channels + ch]; });
                pooled[vox * channels + ch] = sum / (float)n;
            } else {
                roi_slot_avg_grad(idx, n, pts_num, grad_out[vox * channels + ch],
                                  [&](int p, float g) { atomicAdd(grad_in + (size_t)p * channels + ch, g); });
            }
        }
    }
}

// grad_in[argmax[e], c] += grad_out[e] over every output element, channel fastest
__global__ __launch_bounds__(256) void roiaware_max_grad_kernel(const int* __restrict__ argmax,
                                                                const float* __restrict__ grad_out,
                                                                float* __restrict__ grad_in, int pts_num, int channels,
                                                                size_t total) {
    roi_max_grad(argmax, grad_out, grad_in, pts_num, channels, total);
}

// ---- roipoint_pool3d -------------------------------------------------------------------------------------------------------
// The walk both pooling kernels share: the scene in ascending 256-point tiles, every lane testing one point, the tile's hits
// compacted in point order with ballots and a prefix over the four waves, until n_sample indices stand in picked[].
// Returns the workgroup-uniform count (<= n_sample); the caller puts a barrier in front of its first read of picked[].
__device__ __forceinline__ int roipoint_walk(const BoxRec& rec, const float* __restrict__ my_xyz, int pts_num, int n_sample,
                                             int* picked, int (*wave_cnt)[ROI_TILE / 64]) {
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    int cnt = 0, it = 0;                           // workgroup-uniform
    for (int t0 = 0; t0 < pts_num && cnt < n_sample; t0 += ROI_TILE, it ^= 1) {
        const int pt = t0 + tid;
        bool hit = false;
        if (pt < pts_num)
            hit = in_box_rec<PDA_FP_CONTRACT != 0>(rec, my_xyz[(size_t)pt * 3 + 0], my_xyz[(size_t)pt * 3 + 1],
                                                  my_xyz[(size_t)pt * 3 + 2]);
        const uint64_t mask = __ballot(hit);
        if (lane == 0) wave_cnt[it][wave] = __popcll(mask);
        __syncthreads();
        int n_hits;
        const int pos = cnt + roi_wave_prefix(wave_cnt[it], wave, n_hits) + __popcll(mask & lanes_below());
        if (hit && pos < n_sample) picked[pos] = pt;
        cnt = min(cnt + n_hits, n_sample);
    }
    return cnt;
}

__global__ __launch_bounds__(256) void roipoint_pool_kernel(const float* __restrict__ xyz, const float* __restrict__ boxes,
                                                            const float* __restrict__ feat, float* __restrict__ pooled,
                                                            int* __restrict__ empty_flag, int pts_num, int boxes_num,
                                                            int channels, int n_sample) {
    extern __shared__ __attribute__((aligned(16))) int picked[];           // n_sample point indices
    __shared__ int wave_cnt[2][ROI_TILE / 64];
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const size_t scene = blockIdx.y, box = scene * boxes_num + blockIdx.x;
    const float* b = boxes + box * 7;
    const BoxRec rec = make_box_rec(b[0], b[1], b[2], b[3], b[4], b[5], b[6], (double)1e-5f);
    const float* my_xyz = xyz + scene * pts_num * 3;
    const int cnt = roipoint_walk(rec, my_xyz, pts_num, n_sample, picked, wave_cnt);
    __syncthreads();
    if (cnt == 0) {
        if (tid == 0) empty_flag[box] = 1;         // the rows stay as the caller filled them
        return;
    }
    const int width = 3 + channels;
    float* rows = pooled + box * n_sample * width;
    const float* my_feat = feat + scene * pts_num * channels;
    for (int k = wave; k < n_sample; k += ROI_TILE / 64) {
        const int p = picked[k % cnt];             // slot k >= cnt repeats slot k % cnt
        float* row = rows + (size_t)k * width;
        for (int j = lane; j < width; j += 64)
            row[j] = j < 3 ? my_xyz[(size_t)p * 3 + j] : my_feat[(size_t)p * channels + (j - 3)];
    }
}

__device__ __forceinline__ bool roi_finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// PointRCNNHead.roipool3d_gpu (pointrcnn_head.py:85-130) in one launch: the same walk on the RoI enlarged here, then every
// slot's row [canonical xyz | score | depth | features] written whole, consecutive lanes on consecutive floats.  An empty
// RoI -- no point inside, or a row that is not finite, which never reaches the box test or cosf / sinf -- zeroes its own
// block, so the output needs no fill.  Every flag is written.
__global__ __launch_bounds__(256) void roipoint_pool_canonical_kernel(const float* __restrict__ xyz, const float* __restrict__ scores,
                                                                      const float* __restrict__ feat, const float* __restrict__ rois,
                                                                      float ex, float ey, float ez, float depth_normalizer,
                                                                      float* __restrict__ pooled, int* __restrict__ empty_flag,
                                                                      int pts_num, int boxes_num, int channels, int n_sample) {
    extern __shared__ __attribute__((aligned(16))) int picked[];           // n_sample point indices
    __shared__ int wave_cnt[2][ROI_TILE / 64];
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const size_t scene = blockIdx.y, box = scene * boxes_num + blockIdx.x;
    const float* b = rois + box * 7;
    float r[7];
    bool sane = true;                              // workgroup-uniform: every lane reads the same row
#pragma unroll
    for (int k = 0; k < 7; ++k) { r[k] = b[k]; sane = sane && roi_finite_bits(r[k]); }
    const int width = 5 + channels;
    float* rows = pooled + box * n_sample * width;
    const float* my_xyz = xyz + scene * pts_num * 3;
    int cnt = 0;
    if (sane) {
        const BoxRec rec = make_box_rec(r[0], r[1], r[2], r[3] + ex, r[4] + ey, r[5] + ez, r[6], (double)1e-5f);
        cnt = roipoint_walk(rec, my_xyz, pts_num, n_sample, picked, wave_cnt);
    }
    __syncthreads();
    if (tid == 0) empty_flag[box] = cnt == 0 ? 1 : 0;
    if (cnt == 0) {
        const size_t total = (size_t)n_sample * width;
        for (size_t e = tid; e < total; e += ROI_TILE) rows[e] = 0.f;
        return;
    }
    const float cosa = cosf(-r[6]), sina = sinf(-r[6]);
    const float* my_scores = scores + scene * pts_num;
    const float* my_feat = feat + scene * pts_num * channels;
    for (int k = wave; k < n_sample; k += ROI_TILE / 64) {
        const int p = picked[k % cnt];             // slot k >= cnt repeats slot k % cnt
        float* row = rows + (size_t)k * width;
        for (int j = lane; j < width; j += 64) {
            float v;
            if (j < 5) {
                const float x = my_xyz[(size_t)p * 3 + 0], y = my_xyz[(size_t)p * 3 + 1], z = my_xyz[(size_t)p * 3 + 2];
                const float dx = x - r[0], dy = y - r[1];
                if (j == 0) v = dx * cosa + dy * (-sina);
                else if (j == 1) v = dx * sina + dy * cosa;
                else if (j == 2) v = z - r[2];
                else if (j == 3) v = my_scores[p];
                else v = sqrtf((x * x + y * y) + z * z) / depth_normalizer - 0.5f;
            } else {
                v = my_feat[(size_t)p * channels + (j - 5)];
            }
            row[j] = v;
        }
    }
}

// ---- points_in_boxes_cpu: the (boxes, points) mask, margin 1e-2, no FMA -----------------------------------------------------
// the host statement of the test, shared by the mask and the count: the record of a box row and the predicate on it
__device__ __forceinline__ BoxRec cpu_box_rec(const float* b) {
    return make_box_rec(b[0], b[1], b[2], b[3], b[4], b[5], b[6], (double)1e-2f);
}
__device__ __forceinline__ bool in_cpu_box(const BoxRec& r, float x, float y, float z) { return in_box_rec<false>(r, x, y, z); }

__global__ __launch_bounds__(256) void points_in_boxes_mask_kernel(const float* __restrict__ boxes,
                                                                   const float* __restrict__ pts, int* __restrict__ out,
                                                                   int boxes_num, int pts_num) {
    __shared__ BoxRec rec[256];
    const int pt = blockIdx.x * 256 + threadIdx.x;
    const bool live = pt < pts_num;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) { x = pts[(size_t)pt * 3 + 0]; y = pts[(size_t)pt * 3 + 1]; z = pts[(size_t)pt * 3 + 2]; }
    for (int k0 = 0; k0 < boxes_num; k0 += 256) {
        const int nk = min(256, boxes_num - k0);
        __syncthreads();
        if ((int)threadIdx.x < nk) {
            const BoxRec r = cpu_box_rec(boxes + (size_t)(k0 + threadIdx.x) * 7);
            rec[threadIdx.x] = r;
        }
        __syncthreads();
        if (live)
            for (int k = 0; k < nk; ++k) out[(size_t)(k0 + k) * pts_num + pt] = in_cpu_box(rec[k], x, y, z) ? 1 : 0;
    }
}

// The points of its scene inside each box, counted: a workgroup owns one box of one scene and walks all the points in
// 256-point tiles; a lane tests the point when its batch column names the scene, the hits are counted by ballot, and the
// four waves' integers are added once at the end.  Integer sums only, no atomics, no mask.
__global__ __launch_bounds__(256) void points_in_boxes_count_kernel(const float* __restrict__ pts, int stride,
                                                                    const float* __restrict__ boxes, int* __restrict__ counts,
                                                                    int pts_num, int boxes_num) {
    __shared__ int wave_cnt[ROI_TILE / 64];
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const int scene = blockIdx.y;
    const size_t box = (size_t)scene * boxes_num + blockIdx.x;
    const BoxRec rec = cpu_box_rec(boxes + box * 7);
    const float scene_f = (float)scene;
    int cnt = 0;                                   // wave-uniform
    for (int t0 = 0; t0 < pts_num; t0 += ROI_TILE) {
        const int pt = t0 + tid;
        bool hit = false;
        if (pt < pts_num) {
            const float* p = pts + (size_t)pt * stride;
            const float bcol = p[0];
            if (!is_nan_bits(bcol) && bcol == scene_f) hit = in_cpu_box(rec, p[1], p[2], p[3]);
        }
        cnt += __popcll(__ballot(hit));
    }
    if (lane == 0) wave_cnt[wave] = cnt;
    __syncthreads();
    if (tid == 0) counts[box] = (wave_cnt[0] + wave_cnt[1]) + (wave_cnt[2] + wave_cnt[3]);
}

inline int roi_group_log(int channels) {
    int wlog = 0;
    while (wlog < 6 && (1 << wlog) < channels) ++wlog;
    return wlog;
}

}  // namespace pda

#define PDA_ROI_GRID(name)                                                                                                    \
    PDA_REQUIRE(out_x >= 1 && out_x <= 255 && out_y >= 1 && out_y <= 255 && out_z >= 1 && out_z <= 255 &&                      \
                    max_pts_each_voxel >= 1 && boxes_num >= 0 && pts_num >= 0 && channels >= 0,                                \
                name ": bad size boxes=%d points=%d channels=%d out=(%d,%d,%d) (each 1..255) max_pts_each_voxel=%d", boxes_num, \
                pts_num, channels, out_x, out_y, out_z, max_pts_each_voxel);                                                   \
    PDA_REQUIRE(pool_method == 0 || pool_method == 1, name ": pool_method %d is neither 0 (max) nor 1 (avg)", pool_method)

PDA_API int pda_roiaware_pool3d_fwd(const float* rois, const float* pts, const float* pts_feature, int32_t* argmax,
                                    int32_t* pts_idx_of_voxels, float* pooled_features, int boxes_num, int pts_num, int channels,
                                    int max_pts_each_voxel, int out_x, int out_y, int out_z, int pool_method,
                                    pda_stream_t stream) {
    PDA_ROI_GRID("pda_roiaware_pool3d_fwd");
    if (boxes_num == 0 || pts_num == 0) return PDA_OK;
    PDA_REQUIRE(rois && pts && pts_idx_of_voxels && (channels == 0 || (pts_feature && argmax && pooled_features)),
                "pda_roiaware_pool3d_fwd: null pointer");
    const int n_vox = out_x * out_y * out_z;
    if (n_vox <= pda::ROI_LDS_VOX)
        hipLaunchKernelGGL(pda::roiaware_collect_kernel<true>, dim3(boxes_num), dim3(256), 0, (hipStream_t)stream, rois, pts,
                           pts_idx_of_voxels, pts_num, out_x, out_y, out_z, max_pts_each_voxel);
    else
        hipLaunchKernelGGL(pda::roiaware_collect_kernel<false>, dim3(boxes_num), dim3(256), 0, (hipStream_t)stream, rois, pts,
                           pts_idx_of_voxels, pts_num, out_x, out_y, out_z, max_pts_each_voxel);
    if (channels > 0) {
        const dim3 grid(boxes_num, pda::divup(n_vox, pda::ROI_TILE));
        const int wlog = pda::roi_group_log(channels);
        if (pool_method == 0)
            hipLaunchKernelGGL(pda::roiaware_pool_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, pts_feature,
                               pts_idx_of_voxels, pooled_features, argmax, nullptr, nullptr, pts_num, channels, n_vox,
                               max_pts_each_voxel, wlog);
        else
            hipLaunchKernelGGL(pda::roiaware_pool_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, pts_feature,
                               pts_idx_of_voxels, pooled_features, argmax, nullptr, nullptr, pts_num, channels, n_vox,
                               max_pts_each_voxel, wlog);
    }
    return pda::check_launch("pda_roiaware_pool3d_fwd");
}

PDA_API int pda_roiaware_pool3d_bwd(const int32_t* pts_idx_of_voxels, const int32_t* argmax, const float* grad_out,
                                    float* grad_in, int boxes_num, int pts_num, int channels, int max_pts_each_voxel, int out_x,
                                    int out_y, int out_z, int pool_method, pda_stream_t stream) {
    PDA_ROI_GRID("pda_roiaware_pool3d_bwd");
    if (boxes_num == 0 || pts_num == 0 || channels == 0) return PDA_OK;
    PDA_REQUIRE(grad_out && grad_in && (pool_method == 0 ? argmax != nullptr : pts_idx_of_voxels != nullptr),
                "pda_roiaware_pool3d_bwd: null pointer");
    const int n_vox = out_x * out_y * out_z;
    if (pool_method == 0) {
        const size_t total = (size_t)boxes_num * n_vox * channels;
        const size_t blocks = (total + 255) / 256;
        hipLaunchKernelGGL(pda::roiaware_max_grad_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                           (hipStream_t)stream, argmax, grad_out, grad_in, pts_num, channels, total);
    } else {
        hipLaunchKernelGGL(pda::roiaware_pool_kernel<2>, dim3(boxes_num, pda::divup(n_vox, pda::ROI_TILE)), dim3(256), 0,
                           (hipStream_t)stream, nullptr, pts_idx_of_voxels, nullptr, nullptr, grad_out, grad_in, pts_num,
                           channels, n_vox, max_pts_each_voxel, pda::roi_group_log(channels));
    }
    return pda::check_launch("pda_roiaware_pool3d_bwd");
}

PDA_API int pda_roipoint_pool3d_fwd(const float* xyz, const float* boxes3d, const float* pts_feature, float* pooled_features,
                                    int32_t* pooled_empty_flag, int batch_size, int pts_num, int boxes_num, int channels,
                                    int sampled_pts_num, pda_stream_t stream) {
    PDA_REQUIRE(batch_size >= 0 && pts_num >= 0 && boxes_num >= 0 && channels >= 0 && sampled_pts_num >= 1,
                "pda_roipoint_pool3d_fwd: bad size batch=%d points=%d boxes=%d channels=%d sampled=%d", batch_size, pts_num,
                boxes_num, channels, sampled_pts_num);
    PDA_REQUIRE(sampled_pts_num <= pda::ROIPOINT_MAX_S, "pda_roipoint_pool3d_fwd: %d sampled points do not fit the %d of LDS",
                sampled_pts_num, pda::ROIPOINT_MAX_S);
    if (batch_size == 0 || pts_num == 0 || boxes_num == 0) return PDA_OK;
    PDA_REQUIRE(batch_size <= 65535, "pda_roipoint_pool3d_fwd: batch %d > 65535", batch_size);
    PDA_REQUIRE(xyz && boxes3d && (pts_feature || channels == 0) && pooled_features && pooled_empty_flag,
                "pda_roipoint_pool3d_fwd: null pointer");
    hipLaunchKernelGGL(pda::roipoint_pool_kernel, dim3(boxes_num, batch_size), dim3(256),
                       (size_t)sampled_pts_num * sizeof(int), (hipStream_t)stream, xyz, boxes3d, pts_feature, pooled_features,
                       pooled_empty_flag, pts_num, boxes_num, channels, sampled_pts_num);
    return pda::check_launch("pda_roipoint_pool3d_fwd");
}

PDA_API int pda_roipoint_pool3d_canonical_fwd(const float* xyz, const float* scores, const float* feat, const float* rois,
                                              const float* extra, float depth_normalizer, float* pooled, int32_t* empty_flag,
                                              int batch, int points, int boxes, int channels, int sampled, pda_stream_t stream) {
    PDA_REQUIRE(batch >= 0 && points >= 0 && boxes >= 0 && channels >= 0 && sampled >= 1,
                "pda_roipoint_pool3d_canonical_fwd: bad size batch=%d points=%d boxes=%d channels=%d sampled=%d", batch, points,
                boxes, channels, sampled);
    PDA_REQUIRE(sampled <= pda::ROIPOINT_MAX_S, "pda_roipoint_pool3d_canonical_fwd: %d sampled points do not fit the %d of LDS",
                sampled, pda::ROIPOINT_MAX_S);
    PDA_REQUIRE(batch <= 65535, "pda_roipoint_pool3d_canonical_fwd: batch %d > 65535", batch);
    if (batch == 0 || boxes == 0) return PDA_OK;
    PDA_REQUIRE(rois && extra && pooled && empty_flag && (points == 0 || (xyz && scores && (feat || channels == 0))),
                "pda_roipoint_pool3d_canonical_fwd: null pointer");
    hipLaunchKernelGGL(pda::roipoint_pool_canonical_kernel, dim3(boxes, batch), dim3(256), (size_t)sampled * sizeof(int),
                       (hipStream_t)stream, xyz, scores, feat, rois, extra[0], extra[1], extra[2], depth_normalizer, pooled,
                       empty_flag, points, boxes, channels, sampled);
    return pda::check_launch("pda_roipoint_pool3d_canonical_fwd");
}

PDA_API int pda_points_in_boxes_mask(const float* boxes, const float* pts, int32_t* mask, int boxes_num, int pts_num,
                                     pda_stream_t stream) {
    PDA_REQUIRE(boxes_num >= 0 && pts_num >= 0, "pda_points_in_boxes_mask: boxes=%d points=%d", boxes_num, pts_num);
    if (boxes_num == 0 || pts_num == 0) return PDA_OK;
    PDA_REQUIRE(boxes && pts && mask, "pda_points_in_boxes_mask: null pointer");
    hipLaunchKernelGGL(pda::points_in_boxes_mask_kernel, dim3(pda::divup(pts_num, 256)), dim3(256), 0, (hipStream_t)stream,
                       boxes, pts, mask, boxes_num, pts_num);
    return pda::check_launch("pda_points_in_boxes_mask");
}

PDA_API int pda_points_in_boxes_count(const float* points, int stride, const float* boxes, int32_t* counts, int pts_num,
                                      int batch_size, int boxes_num, pda_stream_t stream) {
    PDA_REQUIRE(pts_num >= 0 && batch_size >= 0 && boxes_num >= 0 && stride >= 4,
                "pda_points_in_boxes_count: bad size points=%d batch=%d boxes=%d stride=%d (>= 4)", pts_num, batch_size, boxes_num,
                stride);
    if (batch_size == 0 || boxes_num == 0) return PDA_OK;
    PDA_REQUIRE(batch_size <= 65535, "pda_points_in_boxes_count: batch %d > 65535", batch_size);
    PDA_REQUIRE((points || pts_num == 0) && boxes && counts, "pda_points_in_boxes_count: null pointer");
    hipLaunchKernelGGL(pda::points_in_boxes_count_kernel, dim3(boxes_num, batch_size), dim3(256), 0, (hipStream_t)stream, points,
                       stride, boxes, counts, pts_num, boxes_num);
    return pda::check_launch("pda_points_in_boxes_count");
}
