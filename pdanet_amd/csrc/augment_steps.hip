// augment_steps.hip -- the augmentor's steps as an ordered program on the device (include/pda_train.h,
// pda_augment_steps): the world steps of augment.hip as single operations, random_world_translation,
// random_world_frustum_dropout and the four local steps (random_local_translation / _rotation / _scaling /
// _frustum_dropout) of the reference's pcdet/datasets/augmentor/augmentor_utils.py, in the order the yaml lists them,
// then limit_period and prepare_data's class filter.  The input is what pda_augment_paste leaves: the pasted scene with
// its class-0 boxes, untransformed.
//
// A local step walks the scene's boxes in order and tests every point against each box as the points are THEN: a point
// in two boxes moves twice, a point moved into a later box moves again.  A box is changed by its own iteration only, so
// the state of every box in front of every op (the box timeline) follows from the boxes and the draws alone, and a
// point's fate from that point and the timeline: one thread walks one point through every box of every op, from its raw
// row, in registers.  Launches (grids from batch, n_cap and box_slots only):
//   sp_timeline_kernel (B)            : thread i carries box i through the ops and records, for every local op, the
//                                       in-box test of the box as it is then, its draw (draw j of an op belongs to the
//                                       j-th box alive there) and what the op does to a point inside.  Run once per
//                                       world-dropout op and once at the end: stage s stops in front of the s-th
//                                       dropout, whose threshold needs the scene's min / max of y or z at that stage.
//   sp_minmax_kernel   (tiles, B)     : one per world-dropout op: walks every point up to that op and reduces min / max
//                                       (order-independent: an ordered-integer atomicMin / atomicMax).
//   sp_count_kernel    (tiles, B)     : walks every point through the whole program, survivors per tile of 256.
//   sp_scan_kernel     (1)            : tile offsets per scene, packed output offsets of points and boxes, info.
//   sp_write_kernel    (tiles + 1, B) : the walk again, stable ballot / mbcnt scatter of the survivors; the last block of
//                                       a scene copies its final boxes.
// A workgroup stages the box records of one local op through LDS once (12 dwords a box) and every thread reads them in
// box order.
//
// Arithmetic.  The file is built with -ffp-contract=off; every line below is a separately rounded operation, following
// numpy 2.x promotion (NEP 50) for float32 arrays and float32 box rows:
//   * a Python float (np.random.uniform's draw, math.cos's result, MARGIN, 2.0) next to a float32 array or np.float32
//     scalar is weak: it is rounded to float32 and the operation is float32.  So get_points_in_box is
//     cosa = (float)cos((double)-rz), local_x = sx * cosa + sy * (-sina) in float32, limits (float)(dx / 2) + 0.1f and
//     dz / 2, all compared with <=; a local translation adds (float)offset in float32; a local scaling is
//     (x - cx) * (float)s + cx; gt_boxes[idx, 6] += noise is h + (float)noise.
//   * np.random.normal(0, std, 1) is a float64 ARRAY: points[:, a] += offset adds in double and rounds once.
//   * rotate_points_along_z turns its angle into a float32 tensor first: c = cos, s = sin of (float)noise, the matrix is
//     float32, and the product is x' * c + y' * (-s), x' * s + y' * c on the centred point (z' + cz is still rounded).
//   * np.max / np.min of a float32 column are np.float32: the world-dropout threshold max - (float)i * (max - min) is
//     float32, as is the local one (z + dz / 2) - (float)i * dz.
#include "pda_common.h"
#include "ragged_scene.h"
#include "augment_xf.h"

namespace pda {
namespace {

constexpr int SP_TILE = 256;
constexpr int SP_WAVES = SP_TILE / PDA_WAVE;
constexpr int SP_BMAX = 256;                 // boxes per scene
constexpr int SP_MAX_OPS = 32;
constexpr int SP_MAX_DROP = 4;
constexpr int ST_NO_BOX = 1, ST_BAD_CAND = 8;    // next to ragged_scene.h's ST_BAD_OFFSETS / ST_OVER_CAP
enum { OP_FLIP_X = 0, OP_FLIP_Y, OP_ROT, OP_SCALE, OP_TRANS, OP_WDROP, OP_LTRANS, OP_LROT, OP_LSCALE, OP_LDROP, OP_COUNT };
enum { DIR_TOP = 0, DIR_BOTTOM, DIR_LEFT, DIR_RIGHT };

struct Prog {
    int n_ops, n_local, n_drop;
    int8_t code[SP_MAX_OPS], arg[SP_MAX_OPS];
    int8_t idx[SP_MAX_OPS];                  // the local-op index (codes 6..9) or the dropout index (code 5)
};

// one box in front of one local op: the in-box test and what the op does to a point inside
struct LRec {
    float cz, hz, cx, cy, cosa, sina, lim_x, lim_y;
    float p0, p1;                            // translation offset | rotation c, s | scale | dropout threshold
    int32_t alive, pad;
};

struct SceneSt {
    int32_t m, m_out, status, pad;           // boxes walked, boxes written, status bits
};

struct Ws {
    SceneSt* scene;                          // (B)
    uint32_t* mm;                            // (B, 4, 2) ordered-integer min / max of a world dropout
    float* thr;                              // (B, 4) its threshold
    LRec* tl;                                // (B, n_local, slots) the box timeline
    float* fin;                              // (B, slots, 8) the final boxes, compacted
    int32_t* tile;                           // (B, tiles)
};

// float <-> an unsigned key with the same order
__device__ __forceinline__ uint32_t key_of(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the world-dropout threshold of a scene from its min / max (np.float32 arithmetic); a scene without points keeps nothing
__device__ __forceinline__ float wdrop_threshold(int dir, uint32_t kmin, uint32_t kmax, double intensity) {
    const bool upper = dir == DIR_TOP || dir == DIR_LEFT;
    if (kmin > kmax) return upper ? -INFINITY : INFINITY;
    const float mn = float_of(kmin), mx = float_of(kmax);
    const float span = (float)intensity * (mx - mn);
    return upper ? mx - span : mn + span;
}
__device__ __forceinline__ bool wdrop_keeps(int dir, float thr, float y, float z) {
    switch (dir) {
    case DIR_TOP: return z < thr;
    case DIR_BOTTOM: return z > thr;
    case DIR_LEFT: return y < thr;
    default: return y > thr;
    }
}

// the rank of this thread among the flagged threads of the workgroup, and their number (two barriers)
__device__ __forceinline__ int block_rank(bool flag, int32_t* wk, int& total) {
    const uint64_t bk = __ballot(flag);
    const int w = wave_id();
    __syncthreads();
    if (lane_id() == 0) wk[w] = __popcll(bk);
    __syncthreads();
    int r = rank_below(bk);
    total = 0;
    for (int v = 0; v < SP_WAVES; ++v) {
        if (v < w) r += wk[v];
        total += wk[v];
    }
    return r;
}

__device__ __forceinline__ int stop_of(const Prog& pg, int stage) {
    for (int op = 0; op < pg.n_ops; ++op)
        if (pg.code[op] == OP_WDROP && pg.idx[op] == stage) return op;
    return pg.n_ops;
}

// ---- the box timeline ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_BMAX) void sp_timeline_kernel(const float* __restrict__ boxes, const int64_t* __restrict__ boff,
                                                              int64_t m_total, const int64_t* __restrict__ off, int64_t n_total,
                                                              int64_t n_cap, Prog pg, int stage,
                                                              const double* __restrict__ scene_draws,
                                                              const double* __restrict__ box_draws, int draw_cap, int slots,
                                                              Ws ws) {
    __shared__ int32_t wk[SP_WAVES];
    __shared__ int32_t st_sh;
    const int b = blockIdx.x, i = threadIdx.x;
    int st = 0;
    if (!offsets_ok(off, b, n_total) || !offsets_ok(boff, b, m_total)) st |= ST_BAD_OFFSETS;
    else if (off[b + 1] - off[b] > n_cap || boff[b + 1] - boff[b] > slots) st |= ST_OVER_CAP;
    const int m = st ? 0 : (int)(boff[b + 1] - boff[b]);
    if (i == 0) st_sh = st;
    bool alive = i < m;
    float x = 0.f, y = 0.f, z = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, h = 0.f, cls = 0.f;
    if (alive) {
        const float* bx = boxes + (boff[b] + i) * 8;
        x = bx[0]; y = bx[1]; z = bx[2]; dx = bx[3]; dy = bx[4]; dz = bx[5]; h = bx[6]; cls = bx[7];
    }
    int n_alive;
    int rank = block_rank(alive, wk, n_alive);
    const int stop = stop_of(pg, stage);
    const float pi = 3.14159265358979323846f;
    for (int op = 0; op < stop; ++op) {
        const int code = pg.code[op], arg = pg.arg[op];
        const double d = scene_draws[(int64_t)b * pg.n_ops + op];
        if (code == OP_FLIP_X) {
            if (d != 0.0) { y = -y; h = -h; }
        } else if (code == OP_FLIP_Y) {
            if (d != 0.0) { x = -x; h = -(h + pi); }
        } else if (code == OP_ROT) {
            const Xf t = xf_make(0, 0, d, 1.f);
            if (t.rot) { xf_rotate(t.c, t.s, x, y); h = h + t.a; }
        } else if (code == OP_SCALE) {
            const float sc = (float)d;
            x = x * sc; y = y * sc; z = z * sc;
            dx = dx * sc; dy = dy * sc; dz = dz * sc;
        } else if (code == OP_TRANS) {
            if (arg == 0) x = (float)((double)x + d);
            else if (arg == 1) y = (float)((double)y + d);
            else z = (float)((double)z + d);
        } else if (code == OP_WDROP) {
            const int k = pg.idx[op];
            const uint32_t* mm = ws.mm + ((int64_t)b * SP_MAX_DROP + k) * 2;
            const float thr = wdrop_threshold(arg, mm[0], mm[1], d);
            if (i == 0) ws.thr[(int64_t)b * SP_MAX_DROP + k] = thr;
            alive = alive && wdrop_keeps(arg, thr, y, z);       // a box is kept by its centre alone
            rank = block_rank(alive, wk, n_alive);
        } else {
            const int l = pg.idx[op];
            if (i == 0 && n_alive > draw_cap) atomicOr(&st_sh, ST_OVER_CAP);
            double dr = 0.0;
            if (alive && draw_cap > 0) dr = box_draws[((int64_t)b * pg.n_local + l) * draw_cap + min(rank, draw_cap - 1)];
            LRec r;
            r.cx = x; r.cy = y; r.cz = z;
            r.hz = dz / 2.f;
            r.cosa = (float)cos((double)(-h));
            r.sina = (float)sin((double)(-h));
            r.lim_x = dx / 2.f + 0.1f;
            r.lim_y = dy / 2.f + 0.1f;
            r.p0 = r.p1 = 0.f;
            r.alive = alive;
            r.pad = 0;
            const float f = (float)dr;
            if (code == OP_LTRANS) {
                r.p0 = f;
                if (arg == 0) x = x + f;
                else if (arg == 1) y = y + f;
                else z = z + f;
            } else if (code == OP_LROT) {                        // the centre stays: (c - c) rotated is 0, 0 + c is c
                r.p0 = (float)cos((double)f);
                r.p1 = (float)sin((double)f);
                h = h + f;
            } else if (code == OP_LSCALE) {
                r.p0 = f;
                dx = dx * f; dy = dy * f; dz = dz * f;
            } else {                                             // OP_LDROP: the box's own extent on the world axes
                const float span = (arg == DIR_TOP || arg == DIR_BOTTOM) ? dz : dy;
                const float ctr = (arg == DIR_TOP || arg == DIR_BOTTOM) ? z : y;
                const float cut = f * span;
                r.p0 = (arg == DIR_TOP || arg == DIR_LEFT) ? (ctr + span / 2.f) - cut : (ctr - span / 2.f) + cut;
            }
            if (i < m) ws.tl[((int64_t)b * pg.n_local + l) * slots + i] = r;
        }
    }
    if (stage < pg.n_drop) {                                     // the reduction that follows starts from here
        if (i == 0) {
            uint32_t* mm = ws.mm + ((int64_t)b * SP_MAX_DROP + stage) * 2;
            mm[0] = 0xffffffffu;
            mm[1] = 0u;
        }
    } else {                                                     // limit_period, the class filter, the final boxes in order
        const bool keep = alive && cls != 0.f;
        int m_out;
        const int pos = block_rank(keep, wk, m_out);
        if (keep) {
            float* o = ws.fin + ((int64_t)b * slots + pos) * 8;
            o[0] = x; o[1] = y; o[2] = z; o[3] = dx; o[4] = dy; o[5] = dz;
            o[6] = limit_heading(h);
            o[7] = cls;
        }
        __syncthreads();
        if (i == 0) {
            const int s2 = st_sh;
            ws.scene[b] = SceneSt{(s2 & (ST_BAD_OFFSETS | ST_OVER_CAP)) ? 0 : m, (s2 & (ST_BAD_OFFSETS | ST_OVER_CAP)) ? 0 : m_out, s2, 0};
        }
        return;
    }
    __syncthreads();
    if (i == 0) ws.scene[b] = SceneSt{m, 0, st_sh, 0};
}

// ---- the walk of one point -------------------------------------------------------------------------------------------
__device__ __forceinline__ bool in_box(const LRec& r, float x, float y, float z) {
    if (!(fabsf(z - r.cz) <= r.hz)) return false;
    const float sx = x - r.cx, sy = y - r.cy;
    const float lx = sx * r.cosa + sy * (-r.sina);
    const float ly = sx * r.sina + sy * r.cosa;
    return fabsf(lx) <= r.lim_x && fabsf(ly) <= r.lim_y;
}

// Ops [0, stop) on one point.  Every thread of the workgroup calls this with the same stop (the barriers of the LDS
// staging); a point that is not alive walks along and changes nothing.
__device__ __forceinline__ bool walk_point(const Prog& pg, int stop, int b, int m, int slots,
                                           const double* __restrict__ scene_draws, const Ws& ws, LRec* sh, bool alive,
                                           float& x, float& y, float& z) {
    for (int op = 0; op < stop; ++op) {
        const int code = pg.code[op], arg = pg.arg[op];
        const double d = scene_draws[(int64_t)b * pg.n_ops + op];
        if (code == OP_FLIP_X) {
            if (d != 0.0) y = -y;
        } else if (code == OP_FLIP_Y) {
            if (d != 0.0) x = -x;
        } else if (code == OP_ROT) {
            const Xf t = xf_make(0, 0, d, 1.f);
            if (t.rot) xf_rotate(t.c, t.s, x, y);
        } else if (code == OP_SCALE) {
            const float sc = (float)d;
            x = x * sc; y = y * sc; z = z * sc;
        } else if (code == OP_TRANS) {
            if (arg == 0) x = (float)((double)x + d);
            else if (arg == 1) y = (float)((double)y + d);
            else z = (float)((double)z + d);
        } else if (code == OP_WDROP) {
            alive = alive && wdrop_keeps(arg, ws.thr[(int64_t)b * SP_MAX_DROP + pg.idx[op]], y, z);
        } else {
            __syncthreads();
            if ((int)threadIdx.x < m) sh[threadIdx.x] = ws.tl[((int64_t)b * pg.n_local + pg.idx[op]) * slots + threadIdx.x];
            __syncthreads();
            if (!alive) continue;
            for (int i = 0; i < m; ++i) {
                const LRec& r = sh[i];
                if (!r.alive || !in_box(r, x, y, z)) continue;
                if (code == OP_LTRANS) {
                    if (arg == 0) x = x + r.p0;
                    else if (arg == 1) y = y + r.p0;
                    else z = z + r.p0;
                } else if (code == OP_LROT) {
                    x = x - r.cx; y = y - r.cy; z = z - r.cz;
                    xf_rotate(r.p0, r.p1, x, y);
                    x = x + r.cx; y = y + r.cy; z = z + r.cz;
                } else if (code == OP_LSCALE) {
                    x = x - r.cx; y = y - r.cy; z = z - r.cz;
                    x = x * r.p0; y = y * r.p0; z = z * r.p0;
                    x = x + r.cx; y = y + r.cy; z = z + r.cz;
                } else {
                    const bool hit = arg == DIR_TOP ? z >= r.p0 : arg == DIR_BOTTOM ? z <= r.p0 : arg == DIR_LEFT ? y >= r.p0 : y <= r.p0;
                    if (hit) { alive = false; break; }
                }
            }
        }
    }
    return alive;
}

struct PointIn {
    const float* q;
    bool alive;
    float x, y, z;
};

__device__ __forceinline__ PointIn load_point(const float* __restrict__ pts, const int64_t* __restrict__ off, int c, int b, int t,
                                              const SceneSt& sc) {
    PointIn p;
    const bool ok = !(sc.status & (ST_BAD_OFFSETS | ST_OVER_CAP));
    const int64_t s = ok ? off[b] : 0;
    const int n = ok ? (int)(off[b + 1] - s) : 0;
    const int i = t * SP_TILE + (int)threadIdx.x;
    p.alive = i < n;
    p.q = pts + (s + (p.alive ? i : 0)) * (int64_t)c;
    p.x = p.y = p.z = 0.f;
    if (p.alive) { p.x = p.q[0]; p.y = p.q[1]; p.z = p.q[2]; }
    return p;
}

__global__ __launch_bounds__(SP_TILE) void sp_minmax_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off, int c,
                                                            Prog pg, int stage, const double* __restrict__ scene_draws,
                                                            int slots, Ws ws) {
    __shared__ LRec sh[SP_BMAX];
    __shared__ uint32_t mn_sh, mx_sh;
    const int b = blockIdx.y;
    const SceneSt sc = ws.scene[b];
    if (threadIdx.x == 0) { mn_sh = 0xffffffffu; mx_sh = 0u; }
    PointIn p = load_point(pts, off, c, b, blockIdx.x, sc);
    const int stop = stop_of(pg, stage);
    const bool alive = walk_point(pg, stop, b, sc.m, slots, scene_draws, ws, sh, p.alive, p.x, p.y, p.z);
    __syncthreads();
    if (alive) {
        const int dir = pg.arg[stop];
        const uint32_t k = key_of((dir == DIR_TOP || dir == DIR_BOTTOM) ? p.z : p.y);
        atomicMin(&mn_sh, k);
        atomicMax(&mx_sh, k);
    }
    __syncthreads();
    if (threadIdx.x == 0 && mn_sh <= mx_sh) {
        uint32_t* mm = ws.mm + ((int64_t)b * SP_MAX_DROP + stage) * 2;
        atomicMin(mm, mn_sh);
        atomicMax(mm + 1, mx_sh);
    }
}

__global__ __launch_bounds__(SP_TILE) void sp_count_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off, int c,
                                                           Prog pg, const double* __restrict__ scene_draws, int slots,
                                                           int tiles, Ws ws) {
    __shared__ LRec sh[SP_BMAX];
    __shared__ int32_t wk[SP_WAVES];
    const int b = blockIdx.y, t = blockIdx.x;
    const SceneSt sc = ws.scene[b];
    PointIn p = load_point(pts, off, c, b, t, sc);
    const bool alive = walk_point(pg, pg.n_ops, b, sc.m, slots, scene_draws, ws, sh, p.alive, p.x, p.y, p.z);
    int total;
    block_rank(alive, wk, total);
    if (threadIdx.x == 0) ws.tile[(int64_t)b * tiles + t] = total;
}

// One workgroup for the batch: the scenes one after another, each scene's tiles scanned by 1024 threads.
__global__ __launch_bounds__(1024) void sp_scan_kernel(int batch, int tiles, Ws ws, const int32_t* __restrict__ info_in,
                                                       int64_t out_cap, int64_t box_cap, int64_t* __restrict__ out_off,
                                                       int64_t* __restrict__ out_boff, int32_t* __restrict__ info) {
    __shared__ int32_t ps[1024];
    const int u = threadIdx.x;
    const int per = (tiles + 1023) / 1024;
    const int t0 = min(tiles, u * per), t1 = min(tiles, t0 + per);
    int64_t run = 0, brun = 0;
    for (int b = 0; b < batch; ++b) {
        int32_t* tc = ws.tile + (int64_t)b * tiles;
        int32_t sm = 0;
        for (int t = t0; t < t1; ++t) sm += tc[t];
        ps[u] = sm;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {      // Hillis-Steele inclusive scan of the 1024 partial sums
            const int32_t v = u >= o ? ps[u - o] : 0;
            __syncthreads();
            ps[u] += v;
            __syncthreads();
        }
        int32_t r = ps[u] - sm;
        for (int t = t0; t < t1; ++t) {
            const int32_t cnt = tc[t];
            tc[t] = r;
            r += cnt;
        }
        const SceneSt sc = ws.scene[b];
        int status = sc.status;
        if (info_in) status |= info_in[b * 4 + 3] & (ST_BAD_OFFSETS | ST_OVER_CAP | ST_BAD_CAND);
        int64_t n_out = ps[1023], m_out = sc.m_out;
        if (status & (ST_BAD_OFFSETS | ST_OVER_CAP)) n_out = m_out = 0;
        if (run + n_out > out_cap || brun + m_out > box_cap) {
            status |= ST_OVER_CAP;
            n_out = m_out = 0;
        }
        if (n_out == 0 || m_out == 0) status |= ST_NO_BOX;
        __syncthreads();
        if (u == 0) {
            out_off[b] = run;
            out_boff[b] = brun;
            ws.scene[b].status = status;
            info[b * 4 + 0] = (int32_t)n_out;
            info[b * 4 + 1] = (int32_t)m_out;
            info[b * 4 + 2] = (info_in && m_out) ? info_in[b * 4 + 2] : 0;
            info[b * 4 + 3] = status;
        }
        run += n_out;
        brun += m_out;
    }
    if (u == 0) {
        out_off[batch] = run;
        out_boff[batch] = brun;
    }
}

__global__ __launch_bounds__(SP_TILE) void sp_write_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off, int c,
                                                           Prog pg, const double* __restrict__ scene_draws, int slots,
                                                           int tiles, Ws ws, const int64_t* __restrict__ out_off,
                                                           const int64_t* __restrict__ out_boff, float* __restrict__ out,
                                                           float* __restrict__ out_boxes) {
    __shared__ LRec sh[SP_BMAX];
    __shared__ int32_t wk[SP_WAVES];
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int64_t o0 = out_off[b], b0 = out_boff[b];
    const int64_t n_out = out_off[b + 1] - o0, m_out = out_boff[b + 1] - b0;
    if (t == tiles) {                                                      // the final boxes
        const float* fin = ws.fin + (int64_t)b * slots * 8;
        for (int64_t e = tid; e < m_out * 8; e += SP_TILE) out_boxes[b0 * 8 + e] = fin[e];
        return;
    }
    if (n_out == 0) return;                                                // nothing to write (or a flagged scene)
    const SceneSt sc = ws.scene[b];
    PointIn p = load_point(pts, off, c, b, t, sc);
    const bool alive = walk_point(pg, pg.n_ops, b, sc.m, slots, scene_draws, ws, sh, p.alive, p.x, p.y, p.z);
    int total;
    const int r = block_rank(alive, wk, total);
    if (!alive) return;
    float* o = out + (o0 + ws.tile[(int64_t)b * tiles + t] + r) * c;
    o[0] = p.x; o[1] = p.y; o[2] = p.z;
    for (int f = 3; f < c; ++f) o[f] = p.q[f];
}

int64_t al256(int64_t x) { return (x + 255) / 256 * 256; }
bool steps_sizes_ok(int batch, int64_t n_cap, int slots, int n_ops) {
    return batch >= 0 && batch <= 65535 && n_cap >= 1 && n_cap <= (1 << 30) && slots >= 0 && slots <= SP_BMAX && n_ops >= 0 &&
           n_ops <= SP_MAX_OPS;
}

}  // namespace
}  // namespace pda

PDA_API int64_t pda_augment_steps_workspace_bytes(int batch, int64_t n_cap, int box_slots, int n_ops) {
    if (!pda::steps_sizes_ok(batch, n_cap, box_slots, n_ops)) return -1;
    const int64_t slots = box_slots > 0 ? box_slots : 1;
    return pda::al256((int64_t)batch * sizeof(pda::SceneSt)) + pda::al256((int64_t)batch * pda::SP_MAX_DROP * 8) +
           pda::al256((int64_t)batch * pda::SP_MAX_DROP * 4) + pda::al256((int64_t)batch * n_ops * slots * sizeof(pda::LRec)) +
           pda::al256((int64_t)batch * slots * 32) + pda::al256((int64_t)batch * pda::divup64(n_cap, pda::SP_TILE) * 4);
}

PDA_API int pda_augment_steps(const float* points, const int64_t* offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                              const float* boxes, const int64_t* box_offsets, int64_t m_total, const int32_t* ops, int n_ops,
                              const double* scene_draws, const double* box_draws, int draw_cap, int box_slots,
                              const int32_t* info_in, float* out_points, int64_t out_cap, int64_t* out_offsets,
                              float* out_boxes, int64_t out_box_cap, int64_t* out_box_offsets, int32_t* info, void* workspace,
                              pda_stream_t stream) {
    PDA_REQUIRE(pda::steps_sizes_ok(batch, n_cap, box_slots, n_ops) && n_total >= 0 && c >= 3 && c <= 64 && m_total >= 0 &&
                    draw_cap >= 0 && draw_cap <= pda::SP_BMAX && out_cap >= 0 && out_box_cap >= 0,
                "pda_augment_steps: bad size: batch=%d n_total=%lld C=%d n_cap=%lld m_total=%lld n_ops=%d draw_cap=%d "
                "box_slots=%d out_cap=%lld out_box_cap=%lld",
                batch, (long long)n_total, c, (long long)n_cap, (long long)m_total, n_ops, draw_cap, box_slots,
                (long long)out_cap, (long long)out_box_cap);
    PDA_REQUIRE(ops || n_ops == 0, "pda_augment_steps: null pointer");
    pda::Prog pg;
    pg.n_ops = n_ops;
    pg.n_local = pg.n_drop = 0;
    for (int i = 0; i < pda::SP_MAX_OPS; ++i) pg.code[i] = pg.arg[i] = pg.idx[i] = 0;
    for (int i = 0; i < n_ops; ++i) {
        const int code = ops[2 * i], arg = ops[2 * i + 1];
        const bool axis = code == pda::OP_TRANS || code == pda::OP_LTRANS;
        const bool dir = code == pda::OP_WDROP || code == pda::OP_LDROP;
        PDA_REQUIRE(code >= 0 && code < pda::OP_COUNT && arg >= 0 && arg <= (axis ? 2 : dir ? 3 : 0),
                    "pda_augment_steps: bad op %d: code=%d arg=%d", i, code, arg);
        pg.code[i] = (int8_t)code;
        pg.arg[i] = (int8_t)arg;
        if (code == pda::OP_WDROP) pg.idx[i] = (int8_t)pg.n_drop++;
        else if (code >= pda::OP_LTRANS) pg.idx[i] = (int8_t)pg.n_local++;
    }
    PDA_REQUIRE(pg.n_drop <= pda::SP_MAX_DROP, "pda_augment_steps: bad size: %d world dropout ops (at most %d)", pg.n_drop,
                pda::SP_MAX_DROP);
    if (batch == 0) return PDA_OK;
    PDA_REQUIRE(offsets && box_offsets && out_offsets && out_box_offsets && info && workspace && (scene_draws || n_ops == 0) &&
                    (box_draws || pg.n_local == 0 || draw_cap == 0) && (points || n_total == 0) && (boxes || m_total == 0) &&
                    (out_points || out_cap == 0) && (out_boxes || out_box_cap == 0),
                "pda_augment_steps: null pointer");
    const int slots = box_slots > 0 ? box_slots : 1;
    const int tiles = (int)pda::divup64(n_cap, pda::SP_TILE);
    char* w = (char*)workspace;
    pda::Ws ws;
    ws.scene = (pda::SceneSt*)w;
    w += pda::al256((int64_t)batch * sizeof(pda::SceneSt));
    ws.mm = (uint32_t*)w;
    w += pda::al256((int64_t)batch * pda::SP_MAX_DROP * 8);
    ws.thr = (float*)w;
    w += pda::al256((int64_t)batch * pda::SP_MAX_DROP * 4);
    ws.tl = (pda::LRec*)w;
    w += pda::al256((int64_t)batch * n_ops * slots * sizeof(pda::LRec));
    ws.fin = (float*)w;
    w += pda::al256((int64_t)batch * slots * 32);
    ws.tile = (int32_t*)w;
    hipStream_t st = (hipStream_t)stream;
    const dim3 pgrid((unsigned)tiles, (unsigned)batch);
    for (int stage = 0; stage <= pg.n_drop; ++stage) {
        hipLaunchKernelGGL(pda::sp_timeline_kernel, dim3((unsigned)batch), dim3(pda::SP_BMAX), 0, st, boxes, box_offsets, m_total,
                           offsets, n_total, n_cap, pg, stage, scene_draws, box_draws, draw_cap, slots, ws);
        if (stage < pg.n_drop)
            hipLaunchKernelGGL(pda::sp_minmax_kernel, pgrid, dim3(pda::SP_TILE), 0, st, points, offsets, c, pg, stage, scene_draws,
                               slots, ws);
    }
    hipLaunchKernelGGL(pda::sp_count_kernel, pgrid, dim3(pda::SP_TILE), 0, st, points, offsets, c, pg, scene_draws, slots, tiles, ws);
    hipLaunchKernelGGL(pda::sp_scan_kernel, dim3(1), dim3(1024), 0, st, batch, tiles, ws, info_in, out_cap, out_box_cap, out_offsets,
                       out_box_offsets, info);
    hipLaunchKernelGGL(pda::sp_write_kernel, dim3((unsigned)(tiles + 1), (unsigned)batch), dim3(pda::SP_TILE), 0, st, points,
                       offsets, c, pg, scene_draws, slots, tiles, ws, out_offsets, out_box_offsets, out_points, out_boxes);
    return pda::check_launch("pda_augment_steps");
}
