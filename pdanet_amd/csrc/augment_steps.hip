// augment_steps.hip -- the augmentor's steps as an ordered program on the device (include/pda_train.h,
// pda_augment_steps): the world steps of augment.hip as single operations, random_world_translation,
// random_world_frustum_dropout and the four local steps (random_local_translation / _rotation / _scaling /
// _frustum_dropout) of the reference's pcdet/datasets/augmentor/augmentor_utils.py, in the order the yaml lists them,
// then limit_period and prepare_data's class filter.  The input is what pda_augment_paste leaves: the pasted scene with
// its class-0 boxes, untransformed.  random_local_pyramid_aug (pda_pyramid_aug) is at the end of the file: it runs behind a
// program that ends in a hold op, which leaves limit_period and the class filter to it.
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
#include "stage_rng.h"

namespace pda {
namespace {

constexpr int SP_TILE = 256;
constexpr int SP_WAVES = SP_TILE / PDA_WAVE;
constexpr int SP_BMAX = 256;                 // boxes per scene
constexpr int SP_MAX_OPS = 32;
constexpr int SP_MAX_DROP = 4;
constexpr int ST_NO_BOX = 1, ST_BAD_CAND = 8;    // next to ragged_scene.h's ST_BAD_OFFSETS / ST_OVER_CAP
constexpr int ST_BAD_PYR = 16;                   // random_local_pyramid_aug: a short row of draws or an invalid explicit draw
constexpr int ST_EMPTY = ST_BAD_OFFSETS | ST_OVER_CAP | ST_BAD_PYR;    // such a scene is written empty
enum { OP_FLIP_X = 0, OP_FLIP_Y, OP_ROT, OP_SCALE, OP_TRANS, OP_WDROP, OP_LTRANS, OP_LROT, OP_LSCALE, OP_LDROP, OP_COUNT };
constexpr int OP_HOLD = OP_COUNT;                // last op only: no limit_period, no class filter (pda_pyramid_aug follows)
enum { DIR_TOP = 0, DIR_BOTTOM, DIR_LEFT, DIR_RIGHT };

struct Prog {
    int n_ops, n_local, n_drop;
    int hold;                                // the boxes leave as they are: headings not limited, class 0 kept
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

// The boxes a scene leaves with, compacted in order into fin (slots, 8); -> their number.  limit: limit_period on the
// heading (a hold leaves it as it is).  Called by every thread of the workgroup.
__device__ __forceinline__ int final_boxes(bool keep, bool limit, float x, float y, float z, float dx, float dy, float dz, float h,
                                           float cls, float* __restrict__ fin, int32_t* wk) {
    int m_out;
    const int pos = block_rank(keep, wk, m_out);
    if (keep) {
        float* o = fin + (int64_t)pos * 8;
        o[0] = x; o[1] = y; o[2] = z; o[3] = dx; o[4] = dy; o[5] = dz;
        o[6] = limit ? limit_heading(h) : h;
        o[7] = cls;
    }
    return m_out;
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
        const int m_out = final_boxes(alive && (pg.hold || cls != 0.f), !pg.hold, x, y, z, dx, dy, dz, h, cls,
                                      ws.fin + (int64_t)b * slots * 8, wk);
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
    int n;                                   // points of the scene (0 when it is written empty)
    float x, y, z;
};

__device__ __forceinline__ PointIn load_point(const float* __restrict__ pts, const int64_t* __restrict__ off, int c, int b, int t,
                                              const SceneSt& sc) {
    PointIn p;
    const bool ok = !(sc.status & ST_EMPTY);
    const int64_t s = ok ? off[b] : 0;
    p.n = ok ? (int)(off[b + 1] - s) : 0;
    const int i = t * SP_TILE + (int)threadIdx.x;
    p.alive = i < p.n;
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
        if (status & ST_EMPTY) n_out = m_out = 0;
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

// ---- random_local_pyramid_aug (pda_pyramid_aug) --------------------------------------------------------------------------
// The SE-SSD part-aware step of augmentor_utils.py (local_pyramid_dropout -> _sparsify -> _swap).  Each box is six
// pyramids, apex the centre, base a face; a point's pyramid follows from the box frame in closed form (py_face): with
// get_points_in_box's rotation and no margin, u = lx / (dx / 2), v = ly / (dy / 2), w = sz / (dz / 2), inside iff all three
// are within [-1, 1], the face by the largest magnitude and its sign (0 +x, 1 +z, 2 -x, 3 -z, 4 -y, 5 +y, the order of
// get_pyramids).  Launches (grids from batch, n_cap and box_slots only):
//   py_box_kernel    (B)            : thread i is box i: its frame, its draws (dropout for every box, sparsify for the boxes
//                                     left, swap for the boxes left then), the final boxes (limit_period, class filter).
//   py_count1_kernel (tiles, B)     : points of every sparsify-selected pyramid per tile of 256, after the dropout.
//   py_scan1_kernel  (slots, B)     : a workgroup scans one selected box's tile counts: the pyramid's count, thinned iff
//                                     > max, and the validation of an explicit keep list.
//   py_count2_kernel (tiles, B)     : survivors per tile; counts and ordered-integer min / max of the last column for
//                                     the six pyramids of every box left, on the survivors (LDS histogram, then atomics).
//   py_decide_kernel (B)            : thread i is to-swap box i: its face, its partner, whether the pair acts; the frames
//                                     and statistics of both pyramids, the owner of each pyramid.
//   sp_scan_kernel, py_write_kernel : offsets, then the stable scatter with the swap applied.
// A point's rank in a pyramid is the tile's exclusive prefix plus its rank among the tile's threads (ballots in wave
// order), so it is its position in scene order however the scene is tiled.
// Swap arithmetic (float32, as the reference's on float32 rows): corners as boxes_to_corners_3d (dims * +-0.5, c = cos, s =
// sin of the heading, x * c + y * (-s) + cx), surface_center = (((c0 + c1) + c2) + c3) / 4, ratios ((d.x * v.x + d.y * v.y)
// + d.z * v.z) / ((v.x^2 + v.y^2) + v.z^2), the point rebuilt as ((alpha * v0 + beta * v1) + c0) + gamma * v2, the last
// column as (I - min) / clip(max - min, 1e-6, 1) * (max' - min') + min'.
constexpr int PY_KEEP_MAX = 1024;            // SPARSIFY_MAX_NUM at most (the keep list is validated pair by pair)

struct PyBox {
    float cx, cy, cz, cosa, sina, hx, hy, hz;
    int32_t drop_face;                       // the dropped face, or -1
    int32_t sp_face;                         // the face drawn by a sparsify-selected box, or -1
    int32_t sp_slot;                         // its draw index in the sparsify row
    int32_t sp_count;                        // points in that pyramid
    int32_t thin;                            // sp_count > SPARSIFY_MAX_NUM
    int32_t left;                            // index among the boxes in front of the swap, or -1
    int32_t swap_sel, pad;
};

struct PyFrame {
    float c0[3], v0[3], v1[3], sc[3], v2[3], n0, n1, n2, imin, imax;
};

struct PyPair {
    PyFrame a, p;                            // the to-swap pyramid and its partner
    int32_t pyr_a, pyr_p;                    // box * 6 + face
};

struct PyDraws {
    const double* f64;                       // (B, 5, cap): drop u, sparsify u, swap u, swap face u, swap partner u
    const int32_t* i32;                      // (B, 4, cap): drop face, sparsify face, swap face or -1, swap partner or -1
    const uint64_t* key;                     // (B, cap) sparsify keys
    const int32_t* keep;                     // (B, cap, 1 + sp_max): length (0: use the key), ranks; or null
    const int32_t* n;                        // (B, 3) draws in the dropout / sparsify / swap rows
    int cap, sp_max, swap_max;
    double p_drop, p_sp, p_swap;
};

struct PyWs {
    Ws s;                                    // scene, fin and tile, as sp_scan_kernel reads them
    PyBox* box;                              // (B, slots)
    int32_t* sptile;                         // (B, tiles, slots)
    int32_t* cnt;                            // (B, slots * 6)
    uint32_t* mm;                            // (B, slots * 6, 2)
    int32_t* owner;                          // (B, slots * 6) the to-swap box of the pair a pyramid belongs to, or -1
    PyPair* pair;                            // (B, slots)
};

// The rejects in front of the divisions change no answer for a box with positive dimensions (the contract: a box with a
// dimension <= 0 holds no point here, whatever the plain quotients would say): |s| > h * 1.00001f means a quotient above
// 1 + 9e-6, which cannot round to 1.
__device__ __forceinline__ int py_face(const PyBox& r, float x, float y, float z) {
    const float sz = z - r.cz;
    if (fabsf(sz) > r.hz * 1.00001f) return -1;
    const float sx = x - r.cx, sy = y - r.cy;
    const float lx = sx * r.cosa + sy * (-r.sina);
    if (fabsf(lx) > r.hx * 1.00001f) return -1;
    const float ly = sx * r.sina + sy * r.cosa;
    if (fabsf(ly) > r.hy * 1.00001f) return -1;
    const float w = sz / r.hz;
    const float aw = fabsf(w);
    if (!(aw <= 1.f)) return -1;
    const float u = lx / r.hx, v = ly / r.hy;
    const float au = fabsf(u), av = fabsf(v);
    if (!(au <= 1.f && av <= 1.f)) return -1;
    if (au >= av && au >= aw) return u >= 0.f ? 0 : 2;
    if (aw >= av) return w >= 0.f ? 1 : 3;
    return v >= 0.f ? 5 : 4;
}

__global__ __launch_bounds__(SP_BMAX) void py_box_kernel(const float* __restrict__ boxes, const int64_t* __restrict__ boff,
                                                         int64_t m_total, const int64_t* __restrict__ off, int64_t n_total,
                                                         int64_t n_cap, int slots, PyDraws dr, PyWs ws) {
    __shared__ int32_t wk[SP_WAVES];
    __shared__ int32_t st_sh;
    const int b = blockIdx.x, i = threadIdx.x;
    int st = 0;
    if (!offsets_ok(off, b, n_total) || !offsets_ok(boff, b, m_total)) st |= ST_BAD_OFFSETS;
    else if (off[b + 1] - off[b] > n_cap || boff[b + 1] - boff[b] > slots) st |= ST_OVER_CAP;
    const int m = st ? 0 : (int)(boff[b + 1] - boff[b]);
    if (i == 0) st_sh = st;
    const bool alive = i < m;
    float x = 0.f, y = 0.f, z = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, h = 0.f, cls = 0.f;
    if (alive) {
        const float* bx = boxes + (boff[b] + i) * 8;
        x = bx[0]; y = bx[1]; z = bx[2]; dx = bx[3]; dy = bx[4]; dz = bx[5]; h = bx[6]; cls = bx[7];
    }
    const int D = dr.cap;
    const double* f64 = dr.f64 + (int64_t)b * 5 * D;
    const int32_t* i32 = dr.i32 + (int64_t)b * 4 * D;
    const int nd0 = min(dr.n[b * 3], D), nd1 = min(dr.n[b * 3 + 1], D), nd2 = min(dr.n[b * 3 + 2], D);
    bool bad = false;
    PyBox r;
    r.cx = x; r.cy = y; r.cz = z;
    r.cosa = (float)cos((double)(-h));
    r.sina = (float)sin((double)(-h));
    r.hx = dx / 2.f; r.hy = dy / 2.f; r.hz = dz / 2.f;
    r.drop_face = r.sp_face = r.left = -1;
    r.sp_slot = r.sp_count = r.thin = r.swap_sel = r.pad = 0;
    // 1. dropout: every box draws
    if (alive && i < nd0) {
        const int f = i32[i];
        if (f < 0 || f > 5) bad = true;
        else if (f64[i] <= dr.p_drop) r.drop_face = f;
    } else if (alive) bad = true;
    // 2. sparsify: the boxes left draw, in order
    const bool in1 = alive && !bad && r.drop_face < 0;
    int n1;
    const int j1 = block_rank(in1, wk, n1);
    if (in1 && j1 < nd1) {
        const int f = i32[D + j1];
        if (f < 0 || f > 5) bad = true;
        else if (f64[D + j1] <= dr.p_sp) { r.sp_face = f; r.sp_slot = j1; }
    } else if (in1) bad = true;
    // 3. swap: the boxes left then
    const bool in2 = in1 && !bad && r.sp_face < 0;
    int n2;
    const int k = block_rank(in2, wk, n2);
    if (in2 && k < nd2) {
        r.left = k;
        r.swap_sel = f64[2 * D + k] <= dr.p_swap;
    } else if (in2) bad = true;
    if (bad) atomicOr(&st_sh, ST_BAD_PYR);
    // limit_period, the class filter, the final boxes in order
    const int m_out = final_boxes(alive && cls != 0.f, true, x, y, z, dx, dy, dz, h, cls, ws.s.fin + (int64_t)b * slots * 8, wk);
    __syncthreads();
    const int s2 = st_sh;
    const bool empty = s2 & ST_EMPTY;
    if (alive && !empty) ws.box[(int64_t)b * slots + i] = r;
    const int64_t e0 = (int64_t)b * slots * 6;
    for (int e = i; e < slots * 6; e += SP_BMAX) {
        ws.cnt[e0 + e] = 0;
        ws.mm[(e0 + e) * 2] = 0xffffffffu;
        ws.mm[(e0 + e) * 2 + 1] = 0u;
        ws.owner[e0 + e] = -1;
    }
    if (i == 0) ws.s.scene[b] = SceneSt{empty ? 0 : m, empty ? 0 : m_out, s2, 0};
}

__device__ __forceinline__ bool py_dropped(const PyBox* sh, int m, float x, float y, float z) {
    for (int i = 0; i < m; ++i)
        if (sh[i].drop_face >= 0 && py_face(sh[i], x, y, z) == sh[i].drop_face) return true;
    return false;
}

__global__ __launch_bounds__(SP_TILE) void py_count1_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off, int c,
                                                            int slots, int tiles, PyWs ws) {
    __shared__ PyBox sh[SP_BMAX];
    __shared__ int32_t wc[SP_WAVES][SP_BMAX];
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const SceneSt sc = ws.s.scene[b];
    const PointIn p = load_point(pts, off, c, b, t, sc);
    if (t * SP_TILE >= p.n) return;                                        // the whole workgroup: no tile of the scene
    const int m = sc.m;
    if (tid < m) sh[tid] = ws.box[(int64_t)b * slots + tid];
    __syncthreads();
    const bool alive = p.alive && !py_dropped(sh, m, p.x, p.y, p.z);
    const int w = wave_id();
    for (int i = 0; i < m; ++i) {
        if (sh[i].sp_face < 0) continue;
        const uint64_t bk = __ballot(alive && py_face(sh[i], p.x, p.y, p.z) == sh[i].sp_face);
        if (lane_id() == 0) wc[w][i] = __popcll(bk);
    }
    __syncthreads();
    if (tid < m) {
        int s = 0;
        if (sh[tid].sp_face >= 0)
            for (int v = 0; v < SP_WAVES; ++v) s += wc[v][tid];
        ws.sptile[((int64_t)b * tiles + t) * slots + tid] = s;
    }
}

// One workgroup per (box, scene): the tile counts of a sparsify-selected box become exclusive prefixes (256 threads, a run
// of tiles each, a scan of the partial sums in between); the keep list is checked by all threads, entry against entry.
__global__ __launch_bounds__(SP_TILE) void py_scan1_kernel(const int64_t* __restrict__ off, int slots, int tiles, PyDraws dr,
                                                           PyWs ws) {
    __shared__ int32_t ps[SP_TILE];
    const int b = blockIdx.y, i = blockIdx.x, u = threadIdx.x;
    const SceneSt sc = ws.s.scene[b];
    if (i >= sc.m) return;
    PyBox* r = ws.box + (int64_t)b * slots + i;
    const int sp_slot = r->sp_slot;
    if (r->sp_face < 0) return;                                            // the whole workgroup
    const int nt = (int)((off[b + 1] - off[b] + SP_TILE - 1) / SP_TILE);
    const int per = (nt + SP_TILE - 1) / SP_TILE;
    const int t0 = min(nt, u * per), t1 = min(nt, t0 + per);
    int32_t* tc = ws.sptile + (int64_t)b * tiles * slots + i;
    int32_t sm = 0;
    for (int t = t0; t < t1; ++t) sm += tc[(int64_t)t * slots];
    ps[u] = sm;
    __syncthreads();
    for (int o = 1; o < SP_TILE; o <<= 1) {
        const int32_t v = u >= o ? ps[u - o] : 0;
        __syncthreads();
        ps[u] += v;
        __syncthreads();
    }
    int32_t run = ps[u] - sm;
    for (int t = t0; t < t1; ++t) {
        const int32_t cnt = tc[(int64_t)t * slots];
        tc[(int64_t)t * slots] = run;
        run += cnt;
    }
    const int total = ps[SP_TILE - 1];
    const bool thin = total > dr.sp_max;
    if (u == 0) {
        r->sp_count = total;
        r->thin = thin;
    }
    if (!thin || !dr.keep) return;
    const int32_t* kp = dr.keep + ((int64_t)b * dr.cap + sp_slot) * (1 + dr.sp_max);
    if (kp[0] == 0) return;                                                // no list: the key decides
    bool bad = kp[0] != dr.sp_max;
    for (int a = u; a < dr.sp_max && !bad; a += SP_TILE) {
        const int v = kp[1 + a];
        bad = v < 0 || v >= total;
        for (int a2 = 0; a2 < a && !bad; ++a2) bad = kp[1 + a2] == v;
    }
    if (bad) atomicOr(&ws.s.scene[b].status, ST_BAD_PYR);
}

__device__ __forceinline__ bool py_kept(const PyDraws& dr, int b, const PyBox& r, int rank) {
    if (rank >= r.sp_count) return false;                                  // (the bijection is defined below the count only)
    if (dr.keep) {
        const int32_t* kp = dr.keep + ((int64_t)b * dr.cap + r.sp_slot) * (1 + dr.sp_max);
        if (kp[0] != 0) {
            for (int a = 0; a < dr.sp_max; ++a)
                if (kp[1 + a] == rank) return true;
            return false;
        }
    }
    return keyed_bijection(dr.key[(int64_t)b * dr.cap + r.sp_slot], (uint32_t)r.sp_count, (uint32_t)rank) < (uint32_t)dr.sp_max;
}

// Does the point outlive the dropout and the sparsify?  Called by every thread of the workgroup (one barrier).  wb holds,
// per wave and thinned box, the ballot of the wave's lanes inside the box's pyramid.
__device__ __forceinline__ bool py_survives(const PyDraws& dr, const PyBox* sh, int m, int b, int t, int slots, int tiles,
                                            const PyWs& ws, uint64_t (*wb)[SP_BMAX], bool alive, float x, float y, float z) {
    alive = alive && !py_dropped(sh, m, x, y, z);
    const int w = wave_id(), lane = lane_id();
    // every ballot is taken here, in a loop whose branches the whole workgroup takes alike (sh[i].thin is the same for all)
    for (int i = 0; i < m; ++i) {
        if (!sh[i].thin) continue;
        const uint64_t bk = __ballot(alive && py_face(sh[i], x, y, z) == sh[i].sp_face);
        if (lane == 0) wb[w][i] = bk;
    }
    __syncthreads();
    // from here on every lane is on its own: nothing below looks across lanes
    const uint64_t below = (1ull << lane) - 1ull;
    bool in_thin = false, kept = false;
    for (int i = 0; i < m; ++i) {
        if (!sh[i].thin) continue;
        const uint64_t bk = wb[w][i];
        if (!((bk >> lane) & 1ull)) continue;
        int rank = ws.sptile[((int64_t)b * tiles + t) * slots + i] + __popcll(bk & below);
        for (int v = 0; v < w; ++v) rank += __popcll(wb[v][i]);
        in_thin = true;
        if (!kept) kept = py_kept(dr, b, sh[i], rank);
    }
    return alive && (!in_thin || kept);
}

__global__ __launch_bounds__(SP_TILE) void py_count2_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off, int c,
                                                            int slots, int tiles, PyDraws dr, PyWs ws) {
    __shared__ PyBox sh[SP_BMAX];
    __shared__ uint64_t wb[SP_WAVES][SP_BMAX];
    __shared__ int32_t wk[SP_WAVES];
    __shared__ int32_t cnt[SP_BMAX * 6];
    __shared__ uint32_t mn[SP_BMAX * 6], mx[SP_BMAX * 6];
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const SceneSt sc = ws.s.scene[b];
    const PointIn p = load_point(pts, off, c, b, t, sc);
    if (t * SP_TILE >= p.n) {
        if (tid == 0) ws.s.tile[(int64_t)b * tiles + t] = 0;
        return;
    }
    const int m = sc.m;
    if (tid < m) sh[tid] = ws.box[(int64_t)b * slots + tid];
    for (int e = tid; e < m * 6; e += SP_TILE) { cnt[e] = 0; mn[e] = 0xffffffffu; mx[e] = 0u; }
    __syncthreads();
    const bool alive = py_survives(dr, sh, m, b, t, slots, tiles, ws, wb, p.alive, p.x, p.y, p.z);
    int total;
    block_rank(alive, wk, total);
    if (tid == 0) ws.s.tile[(int64_t)b * tiles + t] = total;
    if (alive) {
        const uint32_t k = key_of(p.q[c - 1]);
        for (int i = 0; i < m; ++i) {
            if (sh[i].left < 0) continue;
            const int f = py_face(sh[i], p.x, p.y, p.z);
            if (f < 0) continue;
            atomicAdd(&cnt[i * 6 + f], 1);
            atomicMin(&mn[i * 6 + f], k);
            atomicMax(&mx[i * 6 + f], k);
        }
    }
    __syncthreads();
    const int64_t e0 = (int64_t)b * slots * 6;
    for (int e = tid; e < m * 6; e += SP_TILE) {
        if (!cnt[e]) continue;
        atomicAdd(&ws.cnt[e0 + e], cnt[e]);
        atomicMin(&ws.mm[(e0 + e) * 2], mn[e]);
        atomicMax(&ws.mm[(e0 + e) * 2 + 1], mx[e]);
    }
}

// the frame of one pyramid: corners c0, c1, c3 in get_pyramids' order of the face, the surface centre and the apex
__device__ inline PyFrame py_frame(const float* __restrict__ bx, int face, uint32_t kmin, uint32_t kmax) {
    const int order[6][4] = {{0, 1, 5, 4}, {4, 5, 6, 7}, {7, 6, 2, 3}, {3, 2, 1, 0}, {1, 2, 6, 5}, {0, 4, 7, 3}};
    const float tpl[8][3] = {{0.5f, 0.5f, -0.5f}, {0.5f, -0.5f, -0.5f}, {-0.5f, -0.5f, -0.5f}, {-0.5f, 0.5f, -0.5f},
                             {0.5f, 0.5f, 0.5f},  {0.5f, -0.5f, 0.5f},  {-0.5f, -0.5f, 0.5f},  {-0.5f, 0.5f, 0.5f}};
    const float c = (float)cos((double)bx[6]), s = (float)sin((double)bx[6]);
    float cr[4][3];
    for (int k = 0; k < 4; ++k) {
        const float* tp = tpl[order[face][k]];
        const float tx = bx[3] * tp[0], ty = bx[4] * tp[1], tz = bx[5] * tp[2];
        cr[k][0] = (tx * c + ty * (-s)) + bx[0];
        cr[k][1] = (tx * s + ty * c) + bx[1];
        cr[k][2] = tz + bx[2];
    }
    PyFrame f;
    for (int a = 0; a < 3; ++a) {
        f.c0[a] = cr[0][a];
        f.sc[a] = (((cr[0][a] + cr[1][a]) + cr[2][a]) + cr[3][a]) / 4.f;
        f.v0[a] = cr[1][a] - cr[0][a];
        f.v1[a] = cr[3][a] - cr[0][a];
        f.v2[a] = bx[a] - f.sc[a];
    }
    f.n0 = (f.v0[0] * f.v0[0] + f.v0[1] * f.v0[1]) + f.v0[2] * f.v0[2];
    f.n1 = (f.v1[0] * f.v1[0] + f.v1[1] * f.v1[1]) + f.v1[2] * f.v1[2];
    f.n2 = (f.v2[0] * f.v2[0] + f.v2[1] * f.v2[1]) + f.v2[2] * f.v2[2];
    f.imin = float_of(kmin);
    f.imax = float_of(kmax);
    return f;
}

__global__ __launch_bounds__(SP_BMAX) void py_decide_kernel(const float* __restrict__ boxes, const int64_t* __restrict__ boff,
                                                            int slots, PyDraws dr, PyWs ws) {
    __shared__ int32_t face_sh[SP_BMAX], part_sh[SP_BMAX], left_box[SP_BMAX], left_of[SP_BMAX];
    const int b = blockIdx.x, i = threadIdx.x;
    const SceneSt sc = ws.s.scene[b];
    const int m = sc.m;
    int left = -1, sel = 0;
    if (i < m) {
        const PyBox& r = ws.box[(int64_t)b * slots + i];
        left = r.left;
        sel = r.swap_sel;
    }
    left_box[i] = -1;
    left_of[i] = left;
    __syncthreads();
    if (left >= 0) left_box[left] = i;
    const int D = dr.cap;
    const double* f64 = dr.f64 + (int64_t)b * 5 * D;
    const int32_t* i32 = dr.i32 + (int64_t)b * 4 * D;
    const int32_t* cnt = ws.cnt + (int64_t)b * slots * 6;
    bool bad = false;
    // the to-swap face among the box's faces with count > SWAP_MAX_NUM
    int face = -1;
    if (sel) {
        int k = 0, mask = 0;
        for (int f = 0; f < 6; ++f)
            if (cnt[i * 6 + f] > dr.swap_max) { ++k; mask |= 1 << f; }
        const int ov = i32[2 * D + left];
        if (ov >= 0) {
            if (ov < 6 && ((mask >> ov) & 1)) face = ov;
            else bad = true;
        } else if (k > 0) {
            int idx = min((int)(f64[3 * D + left] * (double)k), k - 1);
            for (int f = 0; f < 6; ++f)
                if (((mask >> f) & 1) && idx-- == 0) face = f;
        }
    }
    face_sh[i] = face;
    __syncthreads();
    // the partner: a box left whose face `face` has count > SWAP_MAX_NUM and is no to-swap pyramid; none: the box itself
    int partner = -1;
    if (face >= 0) {
        int k = 0;
        for (int q = 0; q < m; ++q) k += left_of[q] >= 0 && cnt[q * 6 + face] > dr.swap_max && face_sh[q] != face;
        const int ov = i32[3 * D + left];
        if (ov >= 0) {
            const int q = ov < SP_BMAX ? left_box[ov] : -1;
            const bool ok = q >= 0 && (k > 0 ? (cnt[q * 6 + face] > dr.swap_max && face_sh[q] != face) : q == i);
            if (ok) partner = q;
            else bad = true;
        } else if (k == 0) {
            partner = i;
        } else {
            int idx = min((int)(f64[4 * D + left] * (double)k), k - 1);
            for (int q = 0; q < m; ++q)
                if (left_of[q] >= 0 && cnt[q * 6 + face] > dr.swap_max && face_sh[q] != face && idx-- == 0) partner = q;
        }
    }
    part_sh[i] = partner;
    __syncthreads();
    if (bad) atomicOr(&ws.s.scene[b].status, ST_BAD_PYR);
    // pairs in ascending to-swap box order: a self pair and a pair whose partner pyramid an earlier pair took do nothing
    bool active = partner >= 0 && partner != i;
    for (int i2 = 0; i2 < i && active; ++i2) active = !(face_sh[i2] == face && part_sh[i2] == partner);
    if (!active) return;
    const int64_t e0 = (int64_t)b * slots * 6;
    const int pa = i * 6 + face, pp = partner * 6 + face;
    ws.owner[e0 + pa] = i;
    ws.owner[e0 + pp] = i;
    ws.s.scene[b].pad = 1;                                                 // the scene has a pair that acts
    PyPair pr;
    pr.a = py_frame(boxes + (boff[b] + i) * 8, face, ws.mm[(e0 + pa) * 2], ws.mm[(e0 + pa) * 2 + 1]);
    pr.p = py_frame(boxes + (boff[b] + partner) * 8, face, ws.mm[(e0 + pp) * 2], ws.mm[(e0 + pp) * 2 + 1]);
    pr.pyr_a = pa;
    pr.pyr_p = pp;
    ws.pair[(int64_t)b * slots + i] = pr;
}

__device__ __forceinline__ float py_dot(float ax, float ay, float az, const float* v) { return (ax * v[0] + ay * v[1]) + az * v[2]; }

// the point of pyramid `from`, by its ratios, in pyramid `to`
__device__ __forceinline__ void py_swap_point(const PyFrame& from, const PyFrame& to, float& x, float& y, float& z, float& in) {
    const float al = py_dot(x - from.c0[0], y - from.c0[1], z - from.c0[2], from.v0) / from.n0;
    const float be = py_dot(x - from.c0[0], y - from.c0[1], z - from.c0[2], from.v1) / from.n1;
    const float ga = py_dot(x - from.sc[0], y - from.sc[1], z - from.sc[2], from.v2) / from.n2;
    x = ((al * to.v0[0] + be * to.v1[0]) + to.c0[0]) + ga * to.v2[0];
    y = ((al * to.v0[1] + be * to.v1[1]) + to.c0[1]) + ga * to.v2[1];
    z = ((al * to.v0[2] + be * to.v1[2]) + to.c0[2]) + ga * to.v2[2];
    const float ratio = (in - from.imin) / fminf(fmaxf(from.imax - from.imin, 1e-6f), 1.f);
    in = ratio * (to.imax - to.imin) + to.imin;
}

__global__ __launch_bounds__(SP_TILE) void py_write_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off, int c,
                                                           int slots, int tiles, PyDraws dr, PyWs ws,
                                                           const int64_t* __restrict__ out_off, const int64_t* __restrict__ out_boff,
                                                           float* __restrict__ out, float* __restrict__ out_boxes) {
    __shared__ PyBox sh[SP_BMAX];
    __shared__ uint64_t wb[SP_WAVES][SP_BMAX];
    __shared__ int32_t wk[SP_WAVES];
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int64_t o0 = out_off[b], b0 = out_boff[b];
    const int64_t n_out = out_off[b + 1] - o0, m_out = out_boff[b + 1] - b0;
    if (t == tiles) {                                                      // the final boxes
        const float* fin = ws.s.fin + (int64_t)b * slots * 8;
        for (int64_t e = tid; e < m_out * 8; e += SP_TILE) out_boxes[b0 * 8 + e] = fin[e];
        return;
    }
    if (n_out == 0) return;                                                // nothing to write (or a flagged scene)
    const SceneSt sc = ws.s.scene[b];
    const PointIn p = load_point(pts, off, c, b, t, sc);
    if (t * SP_TILE >= p.n) return;
    const int m = sc.m;
    if (tid < m) sh[tid] = ws.box[(int64_t)b * slots + tid];
    __syncthreads();
    const bool alive = py_survives(dr, sh, m, b, t, slots, tiles, ws, wb, p.alive, p.x, p.y, p.z);
    int total;
    const int r = block_rank(alive, wk, total);
    if (!alive) return;
    float x = p.x, y = p.y, z = p.z, in = p.q[c - 1];
    if (sc.pad) {                                                          // the first pair with a pyramid that holds the point
        const int32_t* owner = ws.owner + (int64_t)b * slots * 6;
        int own = SP_BMAX, pyr = -1;
        for (int i = 0; i < m; ++i) {
            if (sh[i].left < 0) continue;
            const int f = py_face(sh[i], x, y, z);
            if (f < 0) continue;
            const int o = owner[i * 6 + f];
            if (o >= 0 && o < own) { own = o; pyr = i * 6 + f; }
        }
        if (pyr >= 0) {
            const PyPair& pr = ws.pair[(int64_t)b * slots + own];
            if (pyr == pr.pyr_a) py_swap_point(pr.a, pr.p, x, y, z, in);
            else py_swap_point(pr.p, pr.a, x, y, z, in);
        }
    }
    float* o = out + (o0 + ws.s.tile[(int64_t)b * tiles + t] + r) * c;
    o[0] = x; o[1] = y; o[2] = z;
    for (int f = 3; f < c - 1; ++f) o[f] = p.q[f];
    o[c - 1] = in;
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
    pg.hold = n_ops > 0 && ops[2 * (n_ops - 1)] == pda::OP_HOLD && ops[2 * (n_ops - 1) + 1] == 0;
    n_ops -= pg.hold;                        // the hold is no step (no column in scene_draws), but counts in the 32 ops above
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

PDA_API int64_t pda_pyramid_aug_workspace_bytes(int batch, int64_t n_cap, int box_slots) {
    if (!pda::steps_sizes_ok(batch, n_cap, box_slots, 0)) return -1;
    const int64_t slots = box_slots > 0 ? box_slots : 1, tiles = pda::divup64(n_cap, pda::SP_TILE);
    return pda::al256((int64_t)batch * sizeof(pda::SceneSt)) + pda::al256((int64_t)batch * slots * 32) +
           pda::al256((int64_t)batch * tiles * 4) + pda::al256((int64_t)batch * slots * sizeof(pda::PyBox)) +
           pda::al256((int64_t)batch * tiles * slots * 4) + pda::al256((int64_t)batch * slots * 6 * 4) * 2 +
           pda::al256((int64_t)batch * slots * 6 * 8) + pda::al256((int64_t)batch * slots * sizeof(pda::PyPair));
}

PDA_API int pda_pyramid_aug(const float* points, const int64_t* offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                            const float* boxes, const int64_t* box_offsets, int64_t m_total, const double* draws_f64,
                            const int32_t* draws_i32, const uint64_t* sparsify_key, const int32_t* sparsify_keep,
                            const int32_t* n_draws, int draw_cap, const double* probs, int sparsify_max, int swap_max,
                            int box_slots, const int32_t* info_in, float* out_points, int64_t out_cap, int64_t* out_offsets,
                            float* out_boxes, int64_t out_box_cap, int64_t* out_box_offsets, int32_t* info, void* workspace,
                            pda_stream_t stream) {
    PDA_REQUIRE(pda::steps_sizes_ok(batch, n_cap, box_slots, 0) && n_total >= 0 && c >= 4 && c <= 64 && m_total >= 0 &&
                    draw_cap >= 0 && draw_cap <= pda::SP_BMAX && out_cap >= 0 && out_box_cap >= 0 && sparsify_max >= 0 &&
                    sparsify_max <= pda::PY_KEEP_MAX && swap_max >= 0,
                "pda_pyramid_aug: bad size: batch=%d n_total=%lld C=%d n_cap=%lld m_total=%lld draw_cap=%d box_slots=%d "
                "out_cap=%lld out_box_cap=%lld sparsify_max=%d swap_max=%d",
                batch, (long long)n_total, c, (long long)n_cap, (long long)m_total, draw_cap, box_slots, (long long)out_cap,
                (long long)out_box_cap, sparsify_max, swap_max);
    PDA_REQUIRE(probs, "pda_pyramid_aug: null pointer");
    if (batch == 0) return PDA_OK;
    PDA_REQUIRE(offsets && box_offsets && out_offsets && out_box_offsets && info && workspace && n_draws &&
                    ((draws_f64 && draws_i32 && sparsify_key) || draw_cap == 0) && (points || n_total == 0) &&
                    (boxes || m_total == 0) && (out_points || out_cap == 0) && (out_boxes || out_box_cap == 0),
                "pda_pyramid_aug: null pointer");
    const int slots = box_slots > 0 ? box_slots : 1;
    const int tiles = (int)pda::divup64(n_cap, pda::SP_TILE);
    char* w = (char*)workspace;
    pda::PyWs ws;
    ws.s.mm = nullptr;
    ws.s.thr = nullptr;
    ws.s.tl = nullptr;
    ws.s.scene = (pda::SceneSt*)w;
    w += pda::al256((int64_t)batch * sizeof(pda::SceneSt));
    ws.s.fin = (float*)w;
    w += pda::al256((int64_t)batch * slots * 32);
    ws.s.tile = (int32_t*)w;
    w += pda::al256((int64_t)batch * tiles * 4);
    ws.box = (pda::PyBox*)w;
    w += pda::al256((int64_t)batch * slots * sizeof(pda::PyBox));
    ws.sptile = (int32_t*)w;
    w += pda::al256((int64_t)batch * tiles * slots * 4);
    ws.cnt = (int32_t*)w;
    w += pda::al256((int64_t)batch * slots * 6 * 4);
    ws.owner = (int32_t*)w;
    w += pda::al256((int64_t)batch * slots * 6 * 4);
    ws.mm = (uint32_t*)w;
    w += pda::al256((int64_t)batch * slots * 6 * 8);
    ws.pair = (pda::PyPair*)w;
    pda::PyDraws dr;
    dr.f64 = draws_f64;
    dr.i32 = draws_i32;
    dr.key = sparsify_key;
    dr.keep = sparsify_keep;
    dr.n = n_draws;
    dr.cap = draw_cap;
    dr.sp_max = sparsify_max;
    dr.swap_max = swap_max;
    dr.p_drop = probs[0];
    dr.p_sp = probs[1];
    dr.p_swap = probs[2];
    hipStream_t st = (hipStream_t)stream;
    const dim3 pgrid((unsigned)tiles, (unsigned)batch), bgrid((unsigned)batch);
    hipLaunchKernelGGL(pda::py_box_kernel, bgrid, dim3(pda::SP_BMAX), 0, st, boxes, box_offsets, m_total, offsets, n_total, n_cap,
                       slots, dr, ws);
    hipLaunchKernelGGL(pda::py_count1_kernel, pgrid, dim3(pda::SP_TILE), 0, st, points, offsets, c, slots, tiles, ws);
    hipLaunchKernelGGL(pda::py_scan1_kernel, dim3((unsigned)slots, (unsigned)batch), dim3(pda::SP_TILE), 0, st, offsets, slots, tiles,
                       dr, ws);
    hipLaunchKernelGGL(pda::py_count2_kernel, pgrid, dim3(pda::SP_TILE), 0, st, points, offsets, c, slots, tiles, dr, ws);
    hipLaunchKernelGGL(pda::py_decide_kernel, bgrid, dim3(pda::SP_BMAX), 0, st, boxes, box_offsets, slots, dr, ws);
    hipLaunchKernelGGL(pda::sp_scan_kernel, dim3(1), dim3(1024), 0, st, batch, tiles, ws.s, info_in, out_cap, out_box_cap,
                       out_offsets, out_box_offsets, info);
    hipLaunchKernelGGL(pda::py_write_kernel, dim3((unsigned)(tiles + 1), (unsigned)batch), dim3(pda::SP_TILE), 0, st, points,
                       offsets, c, slots, tiles, dr, ws, out_offsets, out_box_offsets, out_points, out_boxes);
    return pda::check_launch("pda_pyramid_aug");
}
