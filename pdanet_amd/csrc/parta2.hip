// parta2.hip -- the point-wise pieces of Part-A2 that the reference composes from per-scene boolean masks
// (include/pda_train.h, "Part-A2").
//
// part_assign_targets_kernel : PointHeadTemplate.assign_stack_targets(set_ignore_flag=True, ret_part_labels=True)
//                 (point_head_template.py:49-129) for a RAGGED stacked point set in one launch.  One thread per point; the
//                 scene comes from the point's batch column, so rows may be in any order and scenes may be empty.  A workgroup
//                 serves the scenes its 256 points belong to one after the other (lowest first, found with an integer LDS
//                 minimum): the scene's boxes become LDS records once -- trigonometry in double, rounded to float, as
//                 points_in_boxes.hip does (box_rec.h) -- and every lane of that scene tests them in ascending box order.
//                 Scene-major input costs one round per workgroup, two where a workgroup straddles a scene boundary.
// part_loss_kernel + part_loss_finish_kernel : PointHeadTemplate.get_part_layer_loss (:157-170): binary cross entropy of
//                 sigmoid(logit) against the part labels over the foreground points, its sum and the number of foreground
//                 points in float64 partials added in one fixed order (loss_sums.h); no float atomics, nothing read back.
// pool_*_kernel : the input stage of PartA2FCHead (partA2_head.py:104-197) for the whole batch.  The reference loops over the
//                 scenes with boolean masks, collects each scene's points into the RoIs' voxels twice (once for the avg pool of
//                 the part features, once for the max pool of the point features, a table each), and finds the non-empty voxels
//                 with nonzero().  Here: the scene segments of the stacked points by B + 1 binary searches; ONE collection pass
//                 over all B * N RoIs, each walking its scene's segment and storing global rows (roi_pool_core.h, the walk of
//                 roi_pool.hip); the avg pool of the four part channels [offset * (score >= thresh), score] with the masking done
//                 in the operand read, a voxel being live iff their float32 sum in channel order is not zero; the live voxels
//                 compacted in ascending (roi, x, y, z) with ballots, per-workgroup counts and one scan -- integer work only --
//                 and the max pool with argmax over the live voxels alone, channel on the lane axis.  The backward scatters the
//                 feature rows' gradient through argmax and the part rows' through the avg slots, masked as the forward.
#include "pda_common.h"
#include "box_rec.h"
#include "loss_sums.h"
#include "roi_pool_core.h"

namespace pda {
namespace {

constexpr int PA_THREADS = 256;
constexpr int PA_NO_SCENE = 0x7fffffff;
constexpr int64_t PA_MAX_POINTS = (int64_t)1 << 30;

struct PartBoxRec {
    BoxRec box, ext;          // the box and the box enlarged by extra_width (box_utils.enlarge_box3d: f32 additions)
};

__global__ __launch_bounds__(PA_THREADS) void part_assign_targets_kernel(const float* __restrict__ pts,
                                                                         const float* __restrict__ gt_boxes, float ex, float ey,
                                                                         float ez, int64_t* __restrict__ labels,
                                                                         float* __restrict__ part_labels, int64_t n_points, int b,
                                                                         int t, int single_class) {
    __shared__ PartBoxRec rec[PA_THREADS];
    __shared__ int cur;
    const int64_t p = (int64_t)blockIdx.x * PA_THREADS + threadIdx.x;
    const bool live = p < n_points;
    float x = 0.f, y = 0.f, z = 0.f;
    int scene = -1;
    if (live) {
        const float4 v = load4(pts + p * 4);
        x = v.y; y = v.z; z = v.w;
        // a batch value that is not a number, not an integer or outside [0, b) belongs to no scene: label 0, part labels 0
        if (!is_nan_bits(v.x) && v.x >= 0.f && v.x < (float)b) {
            const int s = (int)v.x;
            if ((float)s == v.x) scene = s;
        }
    }
    bool todo = scene >= 0;
    int64_t lab = 0;
    float px = 0.f, py = 0.f, pz = 0.f;
    for (;;) {
        if (threadIdx.x == 0) cur = PA_NO_SCENE;
        __syncthreads();
        if (todo) atomicMin(&cur, scene);
        __syncthreads();
        const int s = cur;
        if (s == PA_NO_SCENE) break;                                 // the same word in every thread: a uniform exit
        const bool mine = todo && scene == s;
        int ib = -1, ie = -1;
        for (int k0 = 0; k0 < t; k0 += PA_THREADS) {
            const int nk = min(PA_THREADS, t - k0);
            __syncthreads();
            if ((int)threadIdx.x < nk) {
                const float* g = gt_boxes + ((size_t)s * t + k0 + threadIdx.x) * 8;
                PartBoxRec r;
                r.box = make_box_rec(g[0], g[1], g[2], g[3], g[4], g[5], g[6], (double)1e-5f);
                r.ext = r.box;
                const float dxe = g[3] + ex, dye = g[4] + ey, dze = g[5] + ez;
                r.ext.hz = dze * 0.5f;
                r.ext.lim_x = (double)dxe / 2.0 + (double)1e-5f;
                r.ext.lim_y = (double)dye / 2.0 + (double)1e-5f;
                rec[threadIdx.x] = r;
            }
            __syncthreads();
            if (mine && (ib < 0 || ie < 0)) {
                for (int k = 0; k < nk; ++k) {
                    if (ib < 0 && in_box_rec<PDA_FP_CONTRACT != 0>(rec[k].box, x, y, z)) ib = k0 + k;
                    if (ie < 0 && in_box_rec<PDA_FP_CONTRACT != 0>(rec[k].ext, x, y, z)) ie = k0 + k;
                    if (ib >= 0 && ie >= 0) break;
                }
            }
        }
        if (mine) {
            todo = false;
            if (ib >= 0) {
                const float4* row = reinterpret_cast<const float4*>(gt_boxes + ((size_t)s * t + ib) * 8);
                const float4 r0 = row[0], r1 = row[1];               // x y z dx | dy dz heading class
                lab = single_class ? 1 : (int64_t)r1.w;
                // rotate_points_along_z(p - c, -heading) / (dx, dy, dz) + 0.5, float32, in that order
                const float sx = x - r0.x, sy = y - r0.y, sz = z - r0.z;
                const float a = -r1.z;
                const float cosa = cosf(a), sina = sinf(a);
                const float rx = sx * cosa + sy * (-sina), ry = sx * sina + sy * cosa;
                px = rx / r0.w + 0.5f;
                py = ry / r1.x + 0.5f;
                pz = sz / r1.y + 0.5f;
            } else if (ie >= 0) {
                lab = -1;                                            // inside an enlarged box only: ignored
            }
        }
        __syncthreads();                                             // everybody has read `cur` before it is reset
    }
    if (live) {
        labels[p] = lab;
        part_labels[p * 3] = px;
        part_labels[p * 3 + 1] = py;
        part_labels[p * 3 + 2] = pz;
    }
}

constexpr int PL_THREADS = 256;
constexpr int PL_PER_THREAD = 4;
constexpr int PL_MAX_BLOCKS = 1024;

// With p = sigmoid(x): bce = -(t * max(log p, -100) + (1 - t) * max(log(1 - p), -100)), torch's clamp.  Evaluated in float64
// from e = exp(-|x|): log p = min(x, 0) - log1p(e), log(1 - p) = min(-x, 0) - log1p(e).  grad (n, 3) is the derivative of that
// clamped expression with respect to x, unscaled; rows that are not foreground get zeros.
__global__ __launch_bounds__(PL_THREADS) void part_loss_kernel(const float* __restrict__ logits, const float* __restrict__ targets,
                                                               const int64_t* __restrict__ labels, float* __restrict__ grad,
                                                               int64_t n_points, double* __restrict__ partials) {
    double s_loss = 0.0, s_pos = 0.0;
    const int64_t stride = (int64_t)gridDim.x * PL_THREADS;
    for (int64_t p = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; p < n_points; p += stride) {
        float g[3] = {0.f, 0.f, 0.f};
        if (labels[p] > 0) {
            s_pos += 1.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double xv = (double)logits[p * 3 + c], tv = (double)targets[p * 3 + c];
                const double e = exp(-fabs(xv));
                const double l1 = log1p(e);
                const double lp = (xv < 0.0 ? xv : 0.0) - l1, lq = (xv > 0.0 ? -xv : 0.0) - l1;
                const double sig = xv >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
                const bool free_p = lp > -100.0, free_q = lq > -100.0;
                s_loss -= tv * (free_p ? lp : -100.0) + (1.0 - tv) * (free_q ? lq : -100.0);
                g[c] = (float)((1.0 - tv) * (free_q ? sig : 0.0) - tv * (free_p ? 1.0 - sig : 0.0));
            }
        }
        grad[p * 3] = g[0];
        grad[p * 3 + 1] = g[1];
        grad[p * 3 + 2] = g[2];
    }
    const double sums[2] = {s_loss, s_pos};
    block_sums_to_partials<2, PL_THREADS>(sums, partials);
}

// out = [loss, scale, #pos]: scale = weight / (3 * max(1, #pos)), loss = scale * the sum; the logit gradient is scale * grad.
__global__ __launch_bounds__(64) void part_loss_finish_kernel(const double* __restrict__ partials, int blocks, double weight,
                                                              float* __restrict__ out) {
    double v[2];
    finish_partials<2>(partials, blocks, v);
    if (threadIdx.x == 0) {
        const double scale = weight / (3.0 * (v[1] > 1.0 ? v[1] : 1.0));
        out[0] = (float)(v[0] * scale);
        out[1] = (float)scale;
        out[2] = (float)v[1];
    }
}

// ---- the RoI head's input stage ---------------------------------------------------------------------------------------------
constexpr int PP_THREADS = ROI_TILE;
constexpr int PP_MAX_OUT = 16;                     // out^3 voxel counters fit ROI_LDS_VOX
constexpr int PP_WAVES = PP_THREADS / 64;

// seg[s], s = 0..b: the first row whose batch value is not below s (a binary search each), so that scene s is rows
// [seg[s], seg[s + 1]) of a scene-major point set.  flag (optional, zeroed by the caller): bit 0 is set when the batch column
// is not ascending or holds a value that names no scene.
__global__ __launch_bounds__(PP_THREADS) void pool_segments_kernel(const float* __restrict__ coords, int n_points, int b,
                                                                   int* __restrict__ seg, int* __restrict__ flag) {
    const int i = blockIdx.x * PP_THREADS + threadIdx.x;
    if (i <= b) {
        int lo = 0, hi = n_points;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (coords[(size_t)mid * 4] < (float)i) lo = mid + 1;
            else hi = mid;
        }
        seg[i] = lo;
    }
    if (flag && i < n_points) {
        const float v = coords[(size_t)i * 4];
        bool bad = is_nan_bits(v) || v < 0.f || !(v < (float)b) || (float)(int)v != v;
        if (i > 0) bad = bad || v < coords[(size_t)(i - 1) * 4];
        if (bad) atomicOr(flag, 1);
    }
}

// One workgroup per RoI of the batch: the walk of roi_pool_core.h over the rows of the RoI's scene, global rows in the slots,
// every voxel's count written (the table needs no fill).
__global__ __launch_bounds__(PP_THREADS) void pool_collect_kernel(const float* __restrict__ rois, const float* __restrict__ coords,
                                                                  const int* __restrict__ seg, int* __restrict__ table, int n_points,
                                                                  int rois_per_scene, int out, int k_slots) {
    __shared__ int cnt[ROI_LDS_VOX];
    __shared__ int hit_vox[ROI_TILE];
    __shared__ int wave_cnt[2][ROI_TILE / 64];
    const int roi = blockIdx.x, scene = roi / rois_per_scene;
    // clamped: a batch column that is not ascending gives wrong segments, never rows outside the point set
    const int p_begin = min(max(seg[scene], 0), n_points), p_end = min(max(seg[scene + 1], p_begin), n_points);
    roi_collect_walk<true, true>(rois + (size_t)roi * 7, coords + 1, 4, p_begin, p_end,
                                 table + (size_t)roi * (out * out * out) * k_slots, out, out, out, k_slots, cnt, hit_vox, wave_cnt);
}

struct PoolPartSrc {
    const float* src;          // point_part_offset (stride 3, offset 0), or with DISABLE_PART point_coords (stride 4, offset 1)
    const float* scores;
    int stride, offset;
    float thresh;
};

// One voxel per thread: the four averaged part channels, the liveness rule, and the workgroup's live mask and count.
__global__ __launch_bounds__(PP_THREADS) void pool_part_kernel(const int* __restrict__ table, PoolPartSrc a,
                                                               float* __restrict__ part_dense, uint64_t* __restrict__ live_bits,
                                                               int* __restrict__ block_cnt, int n_points, int n_vox, int k_slots) {
    __shared__ int wave_cnt[PP_WAVES];
    const int roi = blockIdx.x, v = blockIdx.y * PP_THREADS + threadIdx.x;
    const int blk = roi * gridDim.y + blockIdx.y, lane = lane_id(), wave = wave_id();
    bool live = false;
    if (v < n_vox) {
        const size_t vox = (size_t)roi * n_vox + v;
        const int* idx = table + vox * k_slots;
        const int n = roi_slot_count(idx[0], k_slots);
        if (n > 0) {
            float q[4];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                q[ch] = roi_slot_sum(idx, n, n_points, [&](int p) {
                            return a.scores[p] < a.thresh ? 0.f : a.src[(size_t)p * a.stride + a.offset + ch];
                        }) / (float)n;
            q[3] = roi_slot_sum(idx, n, n_points, [&](int p) { return a.scores[p]; }) / (float)n;
            const float s = ((q[0] + q[1]) + q[2]) + q[3];
            live = (__float_as_uint(s) & 0x7fffffffu) != 0u;        // not +-0; a sum that is not a number counts, as nonzero() counts it
            if (live) store4(part_dense + vox * 4, make_float4(q[0], q[1], q[2], q[3]));
        }
    }
    const uint64_t mask = __ballot(live);
    if (lane == 0) {
        live_bits[(size_t)blk * PP_WAVES + wave] = mask;
        wave_cnt[wave] = __popcll(mask);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < PP_WAVES; ++w) total += wave_cnt[w];
        block_cnt[blk] = total;
    }
}

// One workgroup: block_off = the exclusive prefix of block_cnt, *n_live its total.
__global__ __launch_bounds__(PP_THREADS) void pool_scan_kernel(const int* __restrict__ block_cnt, int* __restrict__ block_off,
                                                               int n_blk, int* __restrict__ n_live) {
    __shared__ int part[PP_THREADS];
    const int tid = threadIdx.x, per = (n_blk + PP_THREADS - 1) / PP_THREADS;
    const int beg = min(tid * per, n_blk), end = min(beg + per, n_blk);
    int s = 0;
    for (int i = beg; i < end; ++i) s += block_cnt[i];
    part[tid] = s;
    __syncthreads();
    int off = 0;
    for (int j = 0; j < tid; ++j) off += part[j];
    for (int i = beg; i < end; ++i) {
        block_off[i] = off;
        off += block_cnt[i];
    }
    if (tid == PP_THREADS - 1) *n_live = off;
}

// The live voxels in ascending (roi, x, y, z): coordinates, part rows and the voxel each row came from.
__global__ __launch_bounds__(PP_THREADS) void pool_compact_kernel(const float* __restrict__ part_dense,
                                                                  const uint64_t* __restrict__ live_bits,
                                                                  const int* __restrict__ block_off, int* __restrict__ coords,
                                                                  float* __restrict__ part_rows, int* __restrict__ live_vox, int n_vox,
                                                                  int out) {
    const int roi = blockIdx.x, v = blockIdx.y * PP_THREADS + threadIdx.x;
    const int blk = roi * gridDim.y + blockIdx.y, lane = lane_id(), wave = wave_id();
    const uint64_t* bits = live_bits + (size_t)blk * PP_WAVES;
    const uint64_t mine = bits[wave];
    if (!((mine >> lane) & 1ull)) return;
    int pos = block_off[blk] + __popcll(mine & lanes_below());
    for (int w = 0; w < wave; ++w) pos += __popcll(bits[w]);
    const size_t vox = (size_t)roi * n_vox + v;
    *reinterpret_cast<int4*>(coords + (size_t)pos * 4) = make_int4(roi, v / (out * out), (v / out) % out, v % out);
    store4(part_rows + (size_t)pos * 4, load4(part_dense + vox * 4));
    live_vox[pos] = (int)vox;
}

// Max pool with argmax over the live voxels: 2^wlog lanes (the channels) per voxel; the grid covers the worst case and the
// rows from *n_live on are left alone.
__global__ __launch_bounds__(PP_THREADS) void pool_features_kernel(const float* __restrict__ feat, const int* __restrict__ table,
                                                                   const int* __restrict__ live_vox, const int* __restrict__ n_live,
                                                                   float* __restrict__ feat_rows, int* __restrict__ arg_rows,
                                                                   int n_points, int channels, int k_slots, int wlog) {
    const int64_t e = ((int64_t)blockIdx.x * PP_THREADS + threadIdx.x) >> wlog;
    if (e >= (int64_t)*n_live) return;
    const int gw = 1 << wlog, j0 = (int)threadIdx.x & (gw - 1);
    const int* idx = table + (size_t)live_vox[e] * k_slots;
    const int n = roi_slot_count(idx[0], k_slots);
    for (int ch = j0; ch < channels; ch += gw) {
        uint32_t bits;
        const int arg = roi_slot_max(feat, idx, n, n_points, channels, ch, bits);
        feat_rows[(size_t)e * channels + ch] = arg != -1 ? __uint_as_float(bits) : 0.f;
        arg_rows[(size_t)e * channels + ch] = arg;
    }
}

__global__ __launch_bounds__(PP_THREADS) void pool_feat_grad_kernel(const int* __restrict__ arg_rows, const float* __restrict__ grad_rows,
                                                                    float* __restrict__ grad_feat, int n_points, int channels,
                                                                    size_t total) {
    roi_max_grad(arg_rows, grad_rows, grad_feat, n_points, channels, total);
}

// grad_offset[p][ch] += grad_part_rows[e][ch] / count for the slots of live voxel e whose point passed the score mask; the score
// channel's gradient is dropped (the reference detaches the scores).
__global__ __launch_bounds__(PP_THREADS) void pool_part_grad_kernel(const int* __restrict__ table, const int* __restrict__ live_vox,
                                                                    const float* __restrict__ scores, float thresh,
                                                                    const float* __restrict__ grad_rows, float* __restrict__ grad_offset,
                                                                    int64_t n_live, int n_points, int k_slots) {
    const int64_t t = (int64_t)blockIdx.x * PP_THREADS + threadIdx.x, e = t >> 2;
    const int ch = (int)(t & 3);
    if (e >= n_live || ch == 3) return;
    const int* idx = table + (size_t)live_vox[e] * k_slots;
    roi_slot_avg_grad(idx, roi_slot_count(idx[0], k_slots), n_points, grad_rows[e * 4 + ch], [&](int p, float g) {
        if (!(scores[p] < thresh)) atomicAdd(grad_offset + (size_t)p * 3 + ch, g);
    });
}

inline bool pool_sizes_ok(int64_t rois_total, int out, int k_slots) {
    return rois_total >= 0 && out >= 1 && out <= PP_MAX_OUT && k_slots >= 1 && k_slots <= 4096 &&
           rois_total * out * out * out < ((int64_t)1 << 31);
}
inline int pool_blocks_y(int out) { return divup(out * out * out, PP_THREADS); }

}  // namespace
}  // namespace pda

PDA_API int pda_part_assign_targets(const float* points, const float* gt_boxes, const float* extra_width, int64_t* labels,
                                    float* part_labels, int64_t n_points, int b, int t, int single_class, pda_stream_t stream) {
    PDA_REQUIRE(n_points >= 0 && n_points <= pda::PA_MAX_POINTS && b >= 1 && b <= (1 << 24) && t >= 0 && (int64_t)b * t < ((int64_t)1 << 27),
                "pda_part_assign_targets: bad size: points=%lld scenes=%d boxes=%d", (long long)n_points, b, t);
    if (n_points == 0) return PDA_OK;
    PDA_REQUIRE(points && extra_width && labels && part_labels && (gt_boxes || t == 0), "pda_part_assign_targets: null pointer");
    PDA_REQUIRE((((uintptr_t)points | (uintptr_t)gt_boxes) & 15) == 0, "pda_part_assign_targets: points / gt_boxes must be 16-byte aligned");
    hipLaunchKernelGGL(pda::part_assign_targets_kernel, dim3((unsigned)pda::divup64(n_points, pda::PA_THREADS)), dim3(pda::PA_THREADS), 0,
                       (hipStream_t)stream, points, gt_boxes, extra_width[0], extra_width[1], extra_width[2], labels, part_labels,
                       n_points, b, t, single_class);
    return pda::check_launch("pda_part_assign_targets");
}

PDA_API int64_t pda_part_loss_blocks(int64_t n_points) {
    if (n_points < 0 || n_points > pda::PA_MAX_POINTS) return -1;
    const int64_t blocks = pda::partial_blocks(n_points, (int64_t)pda::PL_THREADS * pda::PL_PER_THREAD, pda::PL_MAX_BLOCKS);
    return blocks < 1 ? 1 : blocks;
}

PDA_API int pda_part_loss(const float* logits, const float* part_labels, const int64_t* labels, double weight, float* grad,
                          double* partials, float* out, int64_t n_points, pda_stream_t stream) {
    PDA_REQUIRE(n_points >= 0 && n_points <= pda::PA_MAX_POINTS, "pda_part_loss: bad size: points=%lld", (long long)n_points);
    PDA_REQUIRE(partials && out && (n_points == 0 || (logits && part_labels && labels && grad)), "pda_part_loss: null pointer");
    const int blocks = (int)pda_part_loss_blocks(n_points);
    hipLaunchKernelGGL(pda::part_loss_kernel, dim3(blocks), dim3(pda::PL_THREADS), 0, (hipStream_t)stream, logits, part_labels, labels,
                       grad, n_points, partials);
    hipLaunchKernelGGL(pda::part_loss_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partials, blocks, weight, out);
    return pda::check_launch("pda_part_loss");
}

#define PDA_POOL_SIZES(name)                                                                                                  \
    PDA_REQUIRE(pda::pool_sizes_ok(rois_total, out, k_slots) && n_points >= 0 && n_points <= pda::PA_MAX_POINTS,               \
                name ": bad size: rois=%lld points=%lld out=%d (1..%d) max_pts_each_voxel=%d", (long long)rois_total,           \
                (long long)n_points, out, pda::PP_MAX_OUT, k_slots)

PDA_API int64_t pda_parta2_pool_workspace_bytes(int64_t rois_total, int out) {
    if (!pda::pool_sizes_ok(rois_total, out, 1)) return -1;
    const int64_t n_blk = rois_total * pda::pool_blocks_y(out);
    return rois_total * out * out * out * 16 + n_blk * (pda::PP_WAVES * 8 + 8) + 256;
}

PDA_API int pda_parta2_pool_segments(const float* point_coords, int64_t n_points, int b, int32_t* seg, int32_t* flag,
                                     pda_stream_t stream) {
    PDA_REQUIRE(n_points >= 0 && n_points <= pda::PA_MAX_POINTS && b >= 1 && b <= (1 << 24),
                "pda_parta2_pool_segments: bad size: points=%lld scenes=%d", (long long)n_points, b);
    PDA_REQUIRE(seg && (point_coords || n_points == 0), "pda_parta2_pool_segments: null pointer");
    const int64_t threads = n_points > b + 1 ? n_points : b + 1;
    hipLaunchKernelGGL(pda::pool_segments_kernel, dim3((unsigned)pda::divup64(threads, pda::PP_THREADS)), dim3(pda::PP_THREADS), 0,
                       (hipStream_t)stream, point_coords, (int)n_points, b, seg, flag);
    return pda::check_launch("pda_parta2_pool_segments");
}

PDA_API int pda_parta2_pool_collect(const float* rois, const float* point_coords, const int32_t* seg, int32_t* table, int b,
                                    int rois_per_scene, int64_t n_points, int out, int k_slots, pda_stream_t stream) {
    const int64_t rois_total = (int64_t)b * rois_per_scene;
    PDA_REQUIRE(b >= 0 && rois_per_scene >= 0, "pda_parta2_pool_collect: bad size: scenes=%d rois=%d", b, rois_per_scene);
    PDA_POOL_SIZES("pda_parta2_pool_collect");
    if (rois_total == 0) return PDA_OK;
    PDA_REQUIRE(rois && seg && table && (point_coords || n_points == 0), "pda_parta2_pool_collect: null pointer");
    hipLaunchKernelGGL(pda::pool_collect_kernel, dim3((unsigned)rois_total), dim3(pda::PP_THREADS), 0, (hipStream_t)stream, rois,
                       point_coords, seg, table, (int)n_points, rois_per_scene, out, k_slots);
    return pda::check_launch("pda_parta2_pool_collect");
}

PDA_API int pda_parta2_pool_sparsify(const int32_t* table, const float* part_src, int src_stride, int src_offset, const float* scores,
                                     float thresh, void* workspace, int32_t* n_live, int32_t* coords, float* part_rows,
                                     int32_t* live_vox, int64_t rois_total, int64_t n_points, int out, int k_slots,
                                     pda_stream_t stream) {
    PDA_POOL_SIZES("pda_parta2_pool_sparsify");
    PDA_REQUIRE(src_stride >= 3 && src_offset >= 0 && src_offset + 3 <= src_stride, "pda_parta2_pool_sparsify: stride=%d offset=%d",
                src_stride, src_offset);
    PDA_REQUIRE(n_live && workspace, "pda_parta2_pool_sparsify: null pointer");
    const int n_vox = out * out * out, by = pda::pool_blocks_y(out);
    const int64_t n_blk = rois_total * by;
    PDA_REQUIRE(((uintptr_t)workspace & 15) == 0 && (((uintptr_t)coords | (uintptr_t)part_rows) & 15) == 0,
                "pda_parta2_pool_sparsify: workspace / coords / part_rows must be 16-byte aligned");
    float* part_dense = (float*)workspace;
    uint64_t* live_bits = (uint64_t*)(part_dense + rois_total * n_vox * 4);
    int* block_cnt = (int*)(live_bits + n_blk * pda::PP_WAVES);
    int* block_off = block_cnt + n_blk;
    hipStream_t st = (hipStream_t)stream;
    if (rois_total > 0) {
        PDA_REQUIRE(table && coords && part_rows && live_vox && (n_points == 0 || (part_src && scores)),
                    "pda_parta2_pool_sparsify: null pointer");
        const pda::PoolPartSrc a{part_src, scores, src_stride, src_offset, thresh};
        hipLaunchKernelGGL(pda::pool_part_kernel, dim3((unsigned)rois_total, by), dim3(pda::PP_THREADS), 0, st, table, a, part_dense,
                           live_bits, block_cnt, (int)n_points, n_vox, k_slots);
    }
    hipLaunchKernelGGL(pda::pool_scan_kernel, dim3(1), dim3(pda::PP_THREADS), 0, st, block_cnt, block_off, (int)n_blk, n_live);
    if (rois_total > 0)
        hipLaunchKernelGGL(pda::pool_compact_kernel, dim3((unsigned)rois_total, by), dim3(pda::PP_THREADS), 0, st, part_dense, live_bits,
                           block_off, coords, part_rows, live_vox, n_vox, out);
    return pda::check_launch("pda_parta2_pool_sparsify");
}

PDA_API int pda_parta2_pool_features(const float* point_features, const int32_t* table, const int32_t* live_vox, const int32_t* n_live,
                                     float* feat_rows, int32_t* arg_rows, int64_t rois_total, int64_t n_points, int channels, int out,
                                     int k_slots, pda_stream_t stream) {
    PDA_POOL_SIZES("pda_parta2_pool_features");
    PDA_REQUIRE(channels >= 1 && channels <= 4096, "pda_parta2_pool_features: channels=%d", channels);
    const int64_t cap = rois_total * out * out * out;
    if (cap == 0) return PDA_OK;
    PDA_REQUIRE(table && live_vox && n_live && feat_rows && arg_rows && (point_features || n_points == 0),
                "pda_parta2_pool_features: null pointer");
    int wlog = 0;
    while (wlog < 6 && (1 << wlog) < channels) ++wlog;
    hipLaunchKernelGGL(pda::pool_features_kernel, dim3((unsigned)pda::divup64(cap << wlog, pda::PP_THREADS)), dim3(pda::PP_THREADS), 0,
                       (hipStream_t)stream, point_features, table, live_vox, n_live, feat_rows, arg_rows, (int)n_points, channels,
                       k_slots, wlog);
    return pda::check_launch("pda_parta2_pool_features");
}

PDA_API int pda_parta2_pool_bwd(const int32_t* table, const int32_t* live_vox, const int32_t* arg_rows, const float* scores,
                                float thresh, const float* grad_part_rows, const float* grad_feat_rows, float* grad_offset,
                                float* grad_features, int64_t n_live, int64_t n_points, int channels, int k_slots,
                                pda_stream_t stream) {
    PDA_REQUIRE(n_live >= 0 && n_live < ((int64_t)1 << 31) && n_points >= 0 && n_points <= pda::PA_MAX_POINTS && channels >= 1 &&
                    channels <= 4096 && k_slots >= 1 && k_slots <= 4096,
                "pda_parta2_pool_bwd: bad size: rows=%lld points=%lld channels=%d max_pts_each_voxel=%d", (long long)n_live,
                (long long)n_points, channels, k_slots);
    if (n_live == 0 || n_points == 0) return PDA_OK;
    PDA_REQUIRE((!grad_feat_rows || (arg_rows && grad_features)) && (!grad_part_rows || (table && live_vox && scores && grad_offset)),
                "pda_parta2_pool_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (grad_feat_rows) {
        const size_t total = (size_t)n_live * channels, blocks = (total + 255) / 256;
        hipLaunchKernelGGL(pda::pool_feat_grad_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(pda::PP_THREADS), 0, st,
                           arg_rows, grad_feat_rows, grad_features, (int)n_points, channels, total);
    }
    if (grad_part_rows)
        hipLaunchKernelGGL(pda::pool_part_grad_kernel, dim3((unsigned)pda::divup64(n_live * 4, pda::PP_THREADS)), dim3(pda::PP_THREADS), 0,
                           st, table, live_vox, scores, thresh, grad_part_rows, grad_offset, n_live, (int)n_points, k_slots);
    return pda::check_launch("pda_parta2_pool_bwd");
}
