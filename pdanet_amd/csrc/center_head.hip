// center_head.hip -- CenterHead on the device: target assignment, losses and box decoding (dense_heads/center_head.py,
// model_utils/centernet_utils.py, utils/loss_utils.py:395-517).  The pillar scatter in front of it is pillar.hip.
//
// Reference: assign_targets moves every scene's boxes to the host, loops over heads, scenes and boxes in Python and draws
// each Gaussian with numpy; get_loss makes about thirty element-wise passes over the heat maps and reads three scalars back;
// generate_predicted_boxes loops over heads and scenes.
//
// Here: center_targets_kernel, one workgroup per (scene, head, 32 objects): a ballot compaction of the head's rows, the
// target rows, and the Gaussians through an integer atomicMax on the bit pattern; center_focal_kernel +
// center_focal_finish_kernel, one pass over (logits, heat map) with per-workgroup partial sums combined in a fixed order
// (loss_sums.h); center_reg_loss_kernel / center_reg_grad_kernel over the HEAD_ORDER maps as they are; center_decode_kernel
// over the top-K cells of a head.  No float atomics except the one named at center_reg_grad_kernel.
#include "loss_sums.h"

#include <math.h>

namespace pda {
namespace {

// ---- target assignment -------------------------------------------------------------------------------------------------------
constexpr int CH_MAX_HEADS = 8;
constexpr int CH_MAX_CLASSES = 32;
constexpr int CH_MAX_OBJS = 2048;     // NUM_MAX_OBJS: one int32 list in LDS
constexpr int CH_OBJS_PER_BLOCK = 32;
constexpr int CH_THREADS = 256;
constexpr int CH_MAX_CODE = 16;
constexpr int CH_MAX_MAPS = 8;

struct CenterTargetCfg {
    float pcr0, pcr1, vs0, vs1, stride;      // float32 roundings of the Python scalars
    float one_minus, one_plus;               // float32(1 - o), float32(1 + o)
    float b3_scale, c3_scale, a3_four;       // float32(-2 o), float32(o - 1), float32(4 * (4 o))
    int min_radius;
    int num_class, n_heads, H, W, max_objs, cols, m;
    int8_t head_of_class[CH_MAX_CLASSES + 1];   // by label; -1: no head (label 0 is 'bg')
    int8_t local_of_class[CH_MAX_CLASSES + 1];  // index of the class inside its head
    int n_cls[CH_MAX_HEADS];
    float* heatmap[CH_MAX_HEADS];
    float* target_boxes[CH_MAX_HEADS];
    int64_t* inds[CH_MAX_HEADS];
    int64_t* masks[CH_MAX_HEADS];
};

// centernet_utils.gaussian_radius(height, width, min_overlap) as torch evaluates it on float32 tensors
__device__ __forceinline__ float gaussian_radius_f32(float h, float w, const CenterTargetCfg& g) {
    const float hw = h + w;
    const float b1 = hw;
    const float c1 = ((w * h) * g.one_minus) / g.one_plus;
    const float r1 = (b1 + sqrtf(b1 * b1 - 4.f * c1)) / 2.f;
    const float b2 = 2.f * hw;
    const float c2 = (g.one_minus * w) * h;
    const float r2 = (b2 + sqrtf(b2 * b2 - 16.f * c2)) / 2.f;
    const float b3 = g.b3_scale * hw;
    const float c3 = (g.c3_scale * w) * h;
    const float r3 = (b3 + sqrtf(b3 * b3 - g.a3_four * c3)) / 2.f;
    return fminf(fminf(r1, r2), r3);
}

struct CenterObject {
    float coord_x, coord_y;
    int cx, cy, radius, cls;
    bool valid;
};

__device__ __forceinline__ CenterObject center_object(const float* __restrict__ row, const CenterTargetCfg& g) {
    CenterObject o;
    float x = ((row[0] - g.pcr0) / g.vs0) / g.stride;
    float y = ((row[1] - g.pcr1) / g.vs1) / g.stride;
    const float xmax = (float)((double)g.W - 0.5), ymax = (float)((double)g.H - 0.5);
    const bool bad = is_nan_bits(x) || is_nan_bits(y);      // the reference's range test on center_int fails for a NaN
    x = x < 0.f ? 0.f : (x > xmax ? xmax : x);
    y = y < 0.f ? 0.f : (y > ymax ? ymax : y);
    o.coord_x = x;
    o.coord_y = y;
    o.cx = bad ? 0 : (int)x;
    o.cy = bad ? 0 : (int)y;
    const float dx = (row[3] / g.vs0) / g.stride, dy = (row[4] / g.vs1) / g.stride;
    o.valid = !bad && !is_nan_bits(dx) && !is_nan_bits(dy) && dx > 0.f && dy > 0.f;
    int r = g.min_radius;
    if (o.valid) {
        const float rf = gaussian_radius_f32(dx, dy, g);
        // radius.int() of a NaN or of a value beyond int32 is INT_MIN on the host: clamp_min then gives MIN_RADIUS
        if (!is_nan_bits(rf) && rf < 2147483648.f && rf > (float)g.min_radius) r = (int)rf;
    }
    o.radius = r;
    int label = (int)row[g.cols - 1];
    if (label < 0 || label > g.num_class) label = 0;
    o.cls = g.local_of_class[label];
    return o;
}

__global__ __launch_bounds__(CH_THREADS) void center_targets_kernel(const float* __restrict__ gt, CenterTargetCfg g) {
    __shared__ int list[CH_MAX_OBJS];
    __shared__ int n_list;
    const int s = blockIdx.x, h = blockIdx.y, chunk = blockIdx.z;
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const float* sgt = gt + (size_t)s * g.m * g.cols;
    const int K = g.max_objs;
    if (wave == 0) {      // the head's rows in row order; rows beyond NUM_MAX_OBJS are dropped
        int n = 0;
        for (int base = 0; base < g.m && n < K; base += 64) {
            const int i = base + lane;
            bool in = false;
            if (i < g.m) {
                const float lf = sgt[(size_t)i * g.cols + g.cols - 1];
                int label = (lf >= 1.f && lf <= (float)g.num_class) ? (int)lf : 0;
                if (label < 0 || label > g.num_class) label = 0;
                in = g.head_of_class[label] == h;
            }
            const uint64_t mask = __ballot(in);
            const int at = n + rank_below(mask);
            if (in && at < K) list[at] = i;
            n += __popcll(mask);
        }
        if (lane == 0) n_list = min(n, K);
    }
    __syncthreads();
    const int n_obj = n_list;
    const int k0 = chunk * CH_OBJS_PER_BLOCK, k1 = min(k0 + CH_OBJS_PER_BLOCK, K);
    const int code = g.cols;      // cols - 1 box columns, heading as (cos, sin): cols - 1 + 1
    // target rows, indices and masks of this chunk's slots: every slot is written
    for (int k = k0 + (int)threadIdx.x; k < k1; k += CH_THREADS) {
        float* tb = g.target_boxes[h] + ((size_t)s * K + k) * code;
        int64_t ind = 0, msk = 0;
        bool live = false;
        if (k < n_obj) {
            const float* row = sgt + (size_t)list[k] * g.cols;
            const CenterObject o = center_object(row, g);
            if (o.valid) {
                live = true;
                ind = (int64_t)o.cy * g.W + o.cx;
                msk = 1;
                tb[0] = o.coord_x - (float)o.cx;
                tb[1] = o.coord_y - (float)o.cy;
                tb[2] = row[2];
                for (int c = 3; c < 6; ++c) tb[c] = (float)log((double)row[c]);
                tb[6] = (float)cos((double)row[6]);
                tb[7] = (float)sin((double)row[6]);
                for (int c = 8; c < code; ++c) tb[c] = row[c - 1];
            }
        }
        if (!live)
            for (int c = 0; c < code; ++c) tb[c] = 0.f;
        g.inds[h][(size_t)s * K + k] = ind;
        g.masks[h][(size_t)s * K + k] = msk;
    }
    // the Gaussians: one wave per object, lanes over the clipped window; max through the bit pattern (values > 0, map +0)
    for (int k = k0 + wave; k < min(k1, n_obj); k += CH_THREADS / 64) {
        const CenterObject o = center_object(sgt + (size_t)list[k] * g.cols, g);
        if (!o.valid || o.cls < 0 || o.cls >= g.n_cls[h]) continue;
        const int r = o.radius;
        const int left = min(o.cx, r), right = min(g.W - o.cx, r + 1);
        const int top = min(o.cy, r), bottom = min(g.H - o.cy, r + 1);
        const int ww = left + right, wh = top + bottom;
        if (ww <= 0 || wh <= 0) continue;
        const double sigma = (double)(2 * (long long)r + 1) / 6.0;
        const double denom = 2.0 * sigma * sigma;
        int* plane = (int*)(g.heatmap[h] + ((size_t)s * g.n_cls[h] + o.cls) * g.H * g.W);
        const long long cells = (long long)ww * wh;
        for (long long e = lane; e < cells; e += 64) {
            const int j = (int)(e / ww) - top, i = (int)(e % ww) - left;      // offsets from the centre
            const double d2 = (double)i * i + (double)j * j;
            const float v = (float)exp(-d2 / denom);
            atomicMax(plane + (size_t)(o.cy + j) * g.W + (o.cx + i), __float_as_int(v));
        }
    }
}

// ---- heat-map focal loss -----------------------------------------------------------------------------------------------------
constexpr int FL_THREADS = 256;
constexpr int FL_PER_THREAD = 8;
constexpr int FL_MAX_BLOCKS = 1024;

// loss_utils.neg_loss_cornernet on pred = clamp(sigmoid(x), 1e-4, 1 - 1e-4): per workgroup the sums of the positive terms,
// the negative terms and the cells with gt == 1 (partials (3, blocks) float64), and per element the derivative of
// (pos + neg) with respect to x, zero where the clamp is active.
__global__ __launch_bounds__(FL_THREADS) void center_focal_kernel(const float* __restrict__ logits, const float* __restrict__ gt,
                                                                  long long n, float* __restrict__ grad,
                                                                  double* __restrict__ partials) {
    const float lo = 1e-4f, hi = (float)(1.0 - 1e-4);
    double pos = 0.0, neg = 0.0, cnt = 0.0;
    const long long stride = (long long)gridDim.x * FL_THREADS;
    for (long long i = (long long)blockIdx.x * FL_THREADS + threadIdx.x; i < n; i += stride) {
        const float x = logits[i], t = gt[i];
        float p = 1.f / (1.f + expf(-x));
        const bool inside = p >= lo && p <= hi;
        p = p < lo ? lo : (p > hi ? hi : p);
        const double pd = (double)p, q = 1.0 - pd;
        const double dp = inside ? pd * q : 0.0;      // d pred / d x
        double d;
        if (t == 1.f) {
            const double lp = log(pd);
            pos += lp * q * q;
            cnt += 1.0;
            d = q * q / pd - 2.0 * q * lp;
        } else if (t < 1.f) {
            const double w1 = 1.0 - (double)t, w = (w1 * w1) * (w1 * w1), lq = log(q);
            neg += lq * pd * pd * w;
            d = w * (2.0 * pd * lq - pd * pd / q);
        } else {
            d = 0.0;
        }
        grad[i] = (float)(d * dp);
    }
    const double sums[3] = {pos, neg, cnt};
    block_sums_to_partials<3, FL_THREADS>(sums, partials);
}

// out[0] = the loss, out[1] = d loss / d (pos + neg) = -1 / num_pos (-1 without a positive cell), out[2] = num_pos
__global__ __launch_bounds__(64) void center_focal_finish_kernel(const double* __restrict__ partials, int blocks,
                                                                 float* __restrict__ out) {
    double v[3];
    finish_partials<3>(partials, blocks, v);
    if (threadIdx.x == 0) {
        const float pos = (float)v[0], neg = (float)v[1], num = (float)v[2];
        if (num == 0.f) {
            out[0] = 0.f - neg;
            out[1] = -1.f;
        } else {
            out[0] = 0.f - (pos + neg) / num;
            out[1] = -1.f / num;
        }
        out[2] = num;
    }
}

// out = g * (a[0] * b[0] * c): the backward's one scaling pass
__global__ __launch_bounds__(256) void center_scale_kernel(const float* __restrict__ g, const float* __restrict__ a,
                                                           const float* __restrict__ b, float c, long long n,
                                                           float* __restrict__ out) {
    const float s = a[0] * b[0] * c;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) out[i] = g[i] * s;
}

// ---- regression loss ---------------------------------------------------------------------------------------------------------
constexpr int RL_THREADS = 512;

struct CenterMaps {
    const float* map[CH_MAX_MAPS];
    float* grad[CH_MAX_MAPS];
    int channels[CH_MAX_MAPS];
    int n_maps, code;
    float weight[CH_MAX_CODE];      // code_weights
    float loc_weight;
};

// RegLossCenterNet over the HEAD_ORDER maps (each (B, c_i, H * W)) as they are: per code column the sum over (b, k) of
// |pred * m - target * m| with m = mask * not-NaN(target), divided by max(sum(mask), 1).  A masked-out NaN target
// contributes 0 (the reference's 0 * NaN would make the whole column NaN).  One workgroup, sums in a fixed order.
// out: [loc_loss, max(num, 1), reg_loss per column (code)].
__global__ __launch_bounds__(RL_THREADS) void center_reg_loss_kernel(CenterMaps mp, const float* __restrict__ targets,
                                                                     const int64_t* __restrict__ inds,
                                                                     const int64_t* __restrict__ masks, int B, int K,
                                                                     long long hw, float* __restrict__ out) {
    __shared__ double red[RL_THREADS / 64][CH_MAX_CODE + 1];
    double acc[CH_MAX_CODE + 1];
#pragma unroll
    for (int c = 0; c <= CH_MAX_CODE; ++c) acc[c] = 0.0;
    for (int e = threadIdx.x; e < B * K; e += RL_THREADS) {
        const int b = e / K;
        const float m = (float)masks[e];
        acc[CH_MAX_CODE] += (double)m;
        const int64_t ind = inds[e];
        if (m == 0.f || ind < 0 || ind >= hw) continue;
        int col = 0;
        for (int i = 0; i < mp.n_maps; ++i) {
            for (int c = 0; c < mp.channels[i]; ++c, ++col) {
                const float t = targets[(size_t)e * mp.code + col];
                if (is_nan_bits(t)) continue;
                const float p = mp.map[i][((size_t)b * mp.channels[i] + c) * hw + ind];
                const float d = fabsf(p * m - t * m);
#pragma unroll
                for (int q = 0; q < CH_MAX_CODE; ++q)      // a static register index
                    if (q == col) acc[q] += (double)d;
            }
        }
    }
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
#pragma unroll
    for (int c = 0; c <= CH_MAX_CODE; ++c) {
        const double v = wave_sum_f64(acc[c]);
        if (lane == 0) red[wave][c] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double cnt = 0.0;
        for (int w = 0; w < RL_THREADS / 64; ++w) cnt += red[w][CH_MAX_CODE];
        const float num = fmaxf((float)cnt, 1.f);
        float loc = 0.f;
        for (int c = 0; c < mp.code; ++c) {
            double v = 0.0;
            for (int w = 0; w < RL_THREADS / 64; ++w) v += red[w][c];
            const float l = (float)v / num;
            out[2 + c] = l;
            loc += l * mp.weight[c];
        }
        out[0] = loc * mp.loc_weight;
        out[1] = num;
    }
}

// d loc_loss / d map: sign(pred * m - target * m) * m * code_weight * loc_weight / num * grad_out, added to the zero-filled
// map gradients.  The float atomicAdd is needed because two objects can share a cell; a sum of two terms does not depend on
// their order, so the result depends on the execution order only from three objects on one cell on.
__global__ __launch_bounds__(256) void center_reg_grad_kernel(CenterMaps mp, const float* __restrict__ targets,
                                                              const int64_t* __restrict__ inds,
                                                              const int64_t* __restrict__ masks, int B, int K, long long hw,
                                                              const float* __restrict__ fwd_out,
                                                              const float* __restrict__ grad_out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * K) return;
    const int b = e / K;
    const float m = (float)masks[e];
    const int64_t ind = inds[e];
    if (m == 0.f || ind < 0 || ind >= hw) return;
    const float scale = grad_out[0] * mp.loc_weight / fwd_out[1];
    int col = 0;
    for (int i = 0; i < mp.n_maps; ++i) {
        for (int c = 0; c < mp.channels[i]; ++c, ++col) {
            const float t = targets[(size_t)e * mp.code + col];
            if (is_nan_bits(t)) continue;
            const size_t at = ((size_t)b * mp.channels[i] + c) * hw + ind;
            const float d = mp.map[i][at] * m - t * m;
            const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            if (sgn != 0.f) atomicAdd(mp.grad[i] + at, sgn * m * mp.weight[col] * scale);
        }
    }
}

// ---- decoding ----------------------------------------------------------------------------------------------------------------
struct CenterDecodeCfg {
    const float *center, *center_z, *dim, *rot, *vel;      // (B, 2 | 1 | 3 | 2 | 2, H, W); vel may be NULL
    int B, K, H, W, n_cls, use_thresh;
    float stride, vs0, vs1, pcr0, pcr1, thresh;
    float limit[6];
    int32_t class_map[CH_MAX_CLASSES];      // class_id_mapping_each_head of this head
};

// decode_bbox_from_heatmap behind _topk for the K selected cells of every scene: box (7 or 9 columns), score = sigmoid of
// the selected logit or -inf for a row outside POST_CENTER_LIMIT_RANGE / not above SCORE_THRESH, label = mapped class.
__global__ __launch_bounds__(256) void center_decode_kernel(const float* __restrict__ top_logits,
                                                            const int64_t* __restrict__ top_inds, CenterDecodeCfg g,
                                                            float* __restrict__ boxes, float* __restrict__ scores,
                                                            int64_t* __restrict__ labels) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= g.B * g.K) return;
    const int b = e / g.K;
    const long long hw = (long long)g.H * g.W;
    const int cols = g.vel ? 9 : 7;
    float* box = boxes + (size_t)e * cols;
    const int64_t flat = top_inds[e];
    if (flat < 0 || flat >= (int64_t)g.n_cls * hw) {      // never followed
        for (int c = 0; c < cols; ++c) box[c] = 0.f;
        scores[e] = -INFINITY;
        labels[e] = 0;
        return;
    }
    const int cls = (int)(flat / hw);
    const long long cell = flat % hw;
    const float cell_y = (float)(cell / g.W), cell_x = (float)(cell % g.W);
    const float cxo = g.center[((size_t)b * 2 + 0) * hw + cell], cyo = g.center[((size_t)b * 2 + 1) * hw + cell];
    const float rc = g.rot[((size_t)b * 2 + 0) * hw + cell], rs = g.rot[((size_t)b * 2 + 1) * hw + cell];
    const float xs = ((cell_x + cxo) * g.stride) * g.vs0 + g.pcr0;
    const float ys = ((cell_y + cyo) * g.stride) * g.vs1 + g.pcr1;
    const float zs = g.center_z[(size_t)b * hw + cell];
    box[0] = xs;
    box[1] = ys;
    box[2] = zs;
    for (int c = 0; c < 3; ++c) box[3 + c] = (float)exp((double)g.dim[((size_t)b * 3 + c) * hw + cell]);
    box[6] = (float)atan2((double)rs, (double)rc);
    if (g.vel) {
        box[7] = g.vel[((size_t)b * 2 + 0) * hw + cell];
        box[8] = g.vel[((size_t)b * 2 + 1) * hw + cell];
    }
    const float score = 1.f / (1.f + expf(-top_logits[e]));
    bool ok = !is_nan_bits(xs) && !is_nan_bits(ys) && !is_nan_bits(zs) && !is_nan_bits(score);
    ok = ok && xs >= g.limit[0] && ys >= g.limit[1] && zs >= g.limit[2] && xs <= g.limit[3] && ys <= g.limit[4] && zs <= g.limit[5];
    if (g.use_thresh) ok = ok && score > g.thresh;
    scores[e] = ok ? score : -INFINITY;
    labels[e] = g.class_map[cls];
}

}  // namespace
}  // namespace pda

// ---- C entry points ------------------------------------------------------------------------------------------------------------
PDA_API int pda_center_assign_targets(const float* gt_boxes, int gt_cols, int b, int m, int num_class, int n_heads,
                                      const int32_t* head_of_class, const int32_t* local_of_class, const int32_t* head_classes,
                                      int h, int w, int max_objs, double pcr0, double pcr1, double vs0, double vs1,
                                      double stride, double gaussian_overlap, int min_radius, void* const* heatmaps,
                                      void* const* target_boxes, void* const* inds, void* const* masks, pda_stream_t stream) {
    PDA_REQUIRE(b >= 0 && m >= 0 && h >= 0 && w >= 0, "pda_center_assign_targets: b=%d m=%d h=%d w=%d", b, m, h, w);
    PDA_REQUIRE(gt_cols >= 8 && gt_cols <= pda::CH_MAX_CODE, "pda_center_assign_targets: gt_cols=%d outside 8..%d", gt_cols,
                pda::CH_MAX_CODE);
    PDA_REQUIRE(num_class >= 1 && num_class <= pda::CH_MAX_CLASSES, "pda_center_assign_targets: num_class=%d outside 1..%d",
                num_class, pda::CH_MAX_CLASSES);
    PDA_REQUIRE(n_heads >= 1 && n_heads <= pda::CH_MAX_HEADS, "pda_center_assign_targets: n_heads=%d outside 1..%d", n_heads,
                pda::CH_MAX_HEADS);
    PDA_REQUIRE(max_objs >= 1 && max_objs <= pda::CH_MAX_OBJS, "pda_center_assign_targets: max_objs=%d outside 1..%d", max_objs,
                pda::CH_MAX_OBJS);
    PDA_REQUIRE(b <= 65535, "pda_center_assign_targets: batch %d > 65535", b);
    PDA_REQUIRE((int64_t)h * w < ((int64_t)1 << 31), "pda_center_assign_targets: map %d x %d too large", h, w);
    PDA_REQUIRE(vs0 > 0 && vs1 > 0 && stride > 0, "pda_center_assign_targets: voxel size %g, %g or stride %g not positive", vs0,
                vs1, stride);
    PDA_REQUIRE(min_radius >= 0, "pda_center_assign_targets: min_radius=%d < 0", min_radius);
    if (b == 0 || h == 0 || w == 0) return PDA_OK;
    PDA_REQUIRE(head_of_class && local_of_class && head_classes && heatmaps && target_boxes && inds && masks,
                "pda_center_assign_targets: null pointer");
    PDA_REQUIRE(m == 0 || gt_boxes, "pda_center_assign_targets: null gt_boxes");
    pda::CenterTargetCfg g{};
    g.pcr0 = (float)pcr0;
    g.pcr1 = (float)pcr1;
    g.vs0 = (float)vs0;
    g.vs1 = (float)vs1;
    g.stride = (float)stride;
    g.one_minus = (float)(1.0 - gaussian_overlap);
    g.one_plus = (float)(1.0 + gaussian_overlap);
    g.b3_scale = (float)(-2.0 * gaussian_overlap);
    g.c3_scale = (float)(gaussian_overlap - 1.0);
    g.a3_four = (float)(4.0 * (4.0 * gaussian_overlap));
    g.min_radius = min_radius;
    g.num_class = num_class;
    g.n_heads = n_heads;
    g.H = h;
    g.W = w;
    g.max_objs = max_objs;
    g.cols = gt_cols;
    g.m = m;
    g.head_of_class[0] = g.local_of_class[0] = -1;
    for (int c = 1; c <= num_class; ++c) {
        PDA_REQUIRE(head_of_class[c] >= -1 && head_of_class[c] < n_heads, "pda_center_assign_targets: head_of_class[%d]=%d", c,
                    head_of_class[c]);
        PDA_REQUIRE(head_of_class[c] < 0 || (local_of_class[c] >= 0 && local_of_class[c] < head_classes[head_of_class[c]]),
                    "pda_center_assign_targets: local_of_class[%d]=%d", c, local_of_class[c]);
        g.head_of_class[c] = (int8_t)head_of_class[c];
        g.local_of_class[c] = (int8_t)local_of_class[c];
    }
    for (int i = 0; i < n_heads; ++i) {
        PDA_REQUIRE(head_classes[i] >= 1 && head_classes[i] <= num_class, "pda_center_assign_targets: head %d has %d classes", i,
                    head_classes[i]);
        PDA_REQUIRE(heatmaps[i] && target_boxes[i] && inds[i] && masks[i], "pda_center_assign_targets: null output of head %d", i);
        g.n_cls[i] = head_classes[i];
        g.heatmap[i] = (float*)heatmaps[i];
        g.target_boxes[i] = (float*)target_boxes[i];
        g.inds[i] = (int64_t*)inds[i];
        g.masks[i] = (int64_t*)masks[i];
    }
    hipLaunchKernelGGL(pda::center_targets_kernel, dim3(b, n_heads, pda::divup(max_objs, pda::CH_OBJS_PER_BLOCK)),
                       dim3(pda::CH_THREADS), 0, (hipStream_t)stream, gt_boxes, g);
    return pda::check_launch("pda_center_assign_targets");
}

PDA_API int64_t pda_center_focal_blocks(int64_t n) {
    return pda::partial_blocks(n, (int64_t)pda::FL_THREADS * pda::FL_PER_THREAD, pda::FL_MAX_BLOCKS);
}

PDA_API int pda_center_focal_loss(const float* logits, const float* heatmap, int64_t n, float* grad, double* partials,
                                  float* out, pda_stream_t stream) {
    PDA_REQUIRE(n >= 0, "pda_center_focal_loss: n=%lld", (long long)n);
    if (n == 0) return PDA_OK;
    PDA_REQUIRE(logits && heatmap && grad && partials && out, "pda_center_focal_loss: null pointer");
    const int blocks = (int)pda_center_focal_blocks(n);
    hipLaunchKernelGGL(pda::center_focal_kernel, dim3(blocks), dim3(pda::FL_THREADS), 0, (hipStream_t)stream, logits, heatmap,
                       (long long)n, grad, partials);
    hipLaunchKernelGGL(pda::center_focal_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partials, blocks, out);
    return pda::check_launch("pda_center_focal_loss");
}

PDA_API int pda_center_scale(const float* g, const float* a, const float* b, float c, int64_t n, float* out,
                             pda_stream_t stream) {
    PDA_REQUIRE(n >= 0, "pda_center_scale: n=%lld", (long long)n);
    if (n == 0) return PDA_OK;
    PDA_REQUIRE(g && a && b && out, "pda_center_scale: null pointer");
    const int64_t blocks = pda::divup64(n, 256 * 4);
    hipLaunchKernelGGL(pda::center_scale_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                       (hipStream_t)stream, g, a, b, c, (long long)n, out);
    return pda::check_launch("pda_center_scale");
}

static int center_maps(const char* what, pda::CenterMaps& mp, const void* const* maps, void* const* grads, const int32_t* channels,
                       int n_maps, const float* code_weights, float loc_weight, int b, int k, int64_t hw) {
    PDA_REQUIRE(b >= 0 && k >= 0 && hw >= 0 && (int64_t)b * k < ((int64_t)1 << 31), "%s: b=%d k=%d hw=%lld", what, b, k,
                (long long)hw);
    PDA_REQUIRE(n_maps >= 1 && n_maps <= pda::CH_MAX_MAPS, "%s: n_maps=%d outside 1..%d", what, n_maps, pda::CH_MAX_MAPS);
    if ((int64_t)b * k == 0) return PDA_OK;      // the caller returns too
    PDA_REQUIRE(maps && channels && code_weights, "%s: null pointer", what);
    mp.n_maps = n_maps;
    mp.code = 0;
    for (int i = 0; i < n_maps; ++i) {
        PDA_REQUIRE(channels[i] >= 1 && channels[i] <= pda::CH_MAX_CODE, "%s: map %d has %d channels", what, i, channels[i]);
        mp.channels[i] = channels[i];
        mp.code += channels[i];
        mp.map[i] = (const float*)maps[i];
        mp.grad[i] = grads ? (float*)grads[i] : nullptr;
    }
    PDA_REQUIRE(mp.code <= pda::CH_MAX_CODE, "%s: code size %d > %d", what, mp.code, pda::CH_MAX_CODE);
    for (int c = 0; c < mp.code; ++c) mp.weight[c] = code_weights[c];
    mp.loc_weight = loc_weight;
    return PDA_OK;
}

PDA_API int pda_center_reg_loss(const void* const* maps, const int32_t* channels, int n_maps, const float* targets,
                                const int64_t* inds, const int64_t* masks, const float* code_weights, float loc_weight, int b,
                                int k, int64_t hw, float* out, pda_stream_t stream) {
    pda::CenterMaps mp{};
    if (int st = center_maps("pda_center_reg_loss", mp, maps, nullptr, channels, n_maps, code_weights, loc_weight, b, k, hw))
        return st;
    if ((int64_t)b * k == 0) return PDA_OK;
    PDA_REQUIRE(targets && inds && masks && out, "pda_center_reg_loss: null pointer");
    for (int i = 0; i < n_maps; ++i) PDA_REQUIRE(hw == 0 || maps[i], "pda_center_reg_loss: null map %d", i);
    hipLaunchKernelGGL(pda::center_reg_loss_kernel, dim3(1), dim3(pda::RL_THREADS), 0, (hipStream_t)stream, mp, targets, inds,
                       masks, b, k, (long long)hw, out);
    return pda::check_launch("pda_center_reg_loss");
}

PDA_API int pda_center_reg_loss_grad(const void* const* maps, const int32_t* channels, int n_maps, const float* targets,
                                     const int64_t* inds, const int64_t* masks, const float* code_weights, float loc_weight,
                                     int b, int k, int64_t hw, const float* fwd_out, const float* grad_out,
                                     void* const* grad_maps, pda_stream_t stream) {
    pda::CenterMaps mp{};
    if (int st = center_maps("pda_center_reg_loss_grad", mp, maps, grad_maps, channels, n_maps, code_weights, loc_weight, b, k, hw))
        return st;
    if ((int64_t)b * k == 0 || hw == 0) return PDA_OK;
    PDA_REQUIRE(grad_maps && targets && inds && masks && fwd_out && grad_out, "pda_center_reg_loss_grad: null pointer");
    for (int i = 0; i < n_maps; ++i) PDA_REQUIRE(maps[i] && grad_maps[i], "pda_center_reg_loss_grad: null map %d", i);
    hipLaunchKernelGGL(pda::center_reg_grad_kernel, dim3(pda::divup(b * k, 256)), dim3(256), 0, (hipStream_t)stream, mp, targets,
                       inds, masks, b, k, (long long)hw, fwd_out, grad_out);
    return pda::check_launch("pda_center_reg_loss_grad");
}

PDA_API int pda_center_decode(const float* top_logits, const int64_t* top_inds, const float* center, const float* center_z,
                              const float* dim, const float* rot, const float* vel, int b, int k, int h, int w, int n_cls,
                              const int32_t* class_map, double stride, double vs0, double vs1, double pcr0, double pcr1,
                              const float* limit_range, int use_thresh, double score_thresh, float* boxes, float* scores,
                              int64_t* labels, pda_stream_t stream) {
    PDA_REQUIRE(b >= 0 && k >= 0 && h >= 0 && w >= 0 && (int64_t)b * k < ((int64_t)1 << 31), "pda_center_decode: b=%d k=%d h=%d w=%d",
                b, k, h, w);
    PDA_REQUIRE(n_cls >= 1 && n_cls <= pda::CH_MAX_CLASSES, "pda_center_decode: n_cls=%d outside 1..%d", n_cls, pda::CH_MAX_CLASSES);
    PDA_REQUIRE((int64_t)h * w < ((int64_t)1 << 31), "pda_center_decode: map %d x %d too large", h, w);
    if (b == 0 || k == 0) return PDA_OK;
    PDA_REQUIRE(h > 0 && w > 0, "pda_center_decode: empty map with k=%d", k);
    PDA_REQUIRE(top_logits && top_inds && center && center_z && dim && rot && class_map && limit_range && boxes && scores && labels,
                "pda_center_decode: null pointer");
    pda::CenterDecodeCfg g{};
    g.center = center;
    g.center_z = center_z;
    g.dim = dim;
    g.rot = rot;
    g.vel = vel;
    g.B = b;
    g.K = k;
    g.H = h;
    g.W = w;
    g.n_cls = n_cls;
    g.use_thresh = use_thresh ? 1 : 0;
    g.stride = (float)stride;
    g.vs0 = (float)vs0;
    g.vs1 = (float)vs1;
    g.pcr0 = (float)pcr0;
    g.pcr1 = (float)pcr1;
    g.thresh = (float)score_thresh;
    for (int i = 0; i < 6; ++i) g.limit[i] = limit_range[i];
    for (int i = 0; i < n_cls; ++i) g.class_map[i] = class_map[i];
    hipLaunchKernelGGL(pda::center_decode_kernel, dim3(pda::divup(b * k, 256)), dim3(256), 0, (hipStream_t)stream, top_logits,
                       top_inds, g, boxes, scores, labels);
    return pda::check_launch("pda_center_decode");
}
