// augment.hip -- the training-time augmentor on the device (include/pda_train.h, pda_augment): B ragged raw scenes ->
// B ragged augmented scenes in the packed layout pda_input_stage takes next.
//
// Per scene it reproduces the reference's DataAugmentor.forward (pcdet/datasets/augmentor/) for gt_sampling,
// random_world_flip, random_world_rotation and random_world_scaling, followed by limit_period and prepare_data's class
// filter.  The draws come from a host plan: the candidate database objects of every class group (the sampler's pointer /
// permutation bookkeeping stays on the host), the road-plane shift of each candidate, and per scene flip_x, flip_y,
// angle and scale.  Four launches, sized from the batch, n_cap, K and the host-known paste capacity only:
//   ag_select_kernel (B)              : the collision test of DataBaseSampler.__call__.  A candidate is valid iff its BEV
//                                       IoU is 0 with every existing box (of any class), with every other candidate of its
//                                       group (valid or not) and with every valid candidate of an earlier group.  The pair
//                                       tests run in parallel; the group-by-group decision is one bit-mask walk.
//   ag_count_kernel  (tiles, B)       : kept scene points per tile of 256 -- a point is removed when it lies in an
//                                       accepted box enlarged by REMOVE_EXTRA_WIDTH (the CPU test points_in_boxes_cpu).
//   ag_scan_kernel   (1)              : tile offsets per scene, the packed output offsets of points and boxes, info.
//   ag_write_kernel  (tiles + ptiles + 1, B): stable ballot scatter of the kept points, the gather of the pasted object
//                                       points, and the boxes, all through flip -> rotate -> scale (-> limit_period).
// pda_augment_paste is the same four launches in front of the ordered step program (augment_steps.hip): the identity
// transform, the boxes of class 0 kept, no limit_period.
// The file is built with -ffp-contract=off: every product and sum below is a separately rounded float32 (or double)
// operation, as in the reference's numpy / torch CPU code.
#include "pda_common.h"
#include "ragged_scene.h"
#include "bev_overlap.h"
#include "box_rec.h"
#include "augment_xf.h"

namespace pda {
namespace {

constexpr int AG_TILE = 256;
constexpr int AG_WAVES = AG_TILE / PDA_WAVE;
constexpr int AG_KMAX = 256;                 // candidates per scene
constexpr int AG_KWORDS = AG_KMAX / 32;
// info[b][3] status bits of this stage (include/pda_train.h), next to ragged_scene.h's
constexpr int ST_NO_BOX = 1, ST_BAD_CAND = 8;

// per-scene record the select kernel leaves in the workspace
struct SceneRec {
    int32_t n_acc, n_paste, n_keep_boxes, status;
};

struct Db {
    const float* points;      // (n_points, c)
    const int64_t* offsets;   // (n_obj + 1)
    const float* boxes;       // (n_obj, 7)
    const double* centre;     // (n_obj, 3)
    const int32_t* cls;       // (n_obj)
    int64_t n_points;
    int n_obj;
};

struct Plan {
    const int32_t* cand;      // (B, k) database ids, -1 = none
    const int32_t* group;     // (B, k)
    const double* dz;         // (B, k) road-plane shift (mv_height)
    const int32_t* flip;      // (B, 2) flip_x, flip_y
    const double* angle;      // (B)
    const float* scale;       // (B)
    float ew[3];              // REMOVE_EXTRA_WIDTH
    int k;
    int raw;                  // the paste-only form (pda_augment_paste): boxes of class 0 stay, no transform, no limit_period
};

struct Ws {
    SceneRec* scene;          // (B)
    int32_t* acc;             // (B, k) accepted slots, in acceptance order
    int32_t* pfx;             // (B, k + 1) pasted-point prefix of the accepted objects
    int32_t* tile;            // (B, tiles) kept points per tile, then their exclusive scan
};

__device__ __forceinline__ bool object_ok(const Db& db, int id) {
    if (id < 0 || id >= db.n_obj) return false;
    const int64_t s = db.offsets[id], e = db.offsets[id + 1];
    return s >= 0 && e >= s && e <= db.n_points && e - s <= (1 << 30);
}

// ---- the scene transform: flip -> rotate -> scale (augment_xf.h); the paste-only form is the identity ----------------
__device__ __forceinline__ Xf xf_of(const Plan& p, int b) {
    if (p.raw) return xf_make(0, 0, 0.0, 1.f);
    return xf_make(p.flip[2 * b], p.flip[2 * b + 1], p.angle[b], p.scale[b]);
}

// the heading: through the transform and limit_period, or as it is in the paste-only form
__device__ __forceinline__ float heading_of(const Plan& p, const Xf& t, float h) { return p.raw ? h : xf_heading(t, h); }

// the enlarged accepted boxes of scene b as CPU point-test records (margin 1e-2, no FMA)
__device__ int stage_removal_boxes(const Db& db, const Plan& p, const Ws& ws, int b, BoxRec* rec) {
    const int n_acc = ws.scene[b].n_acc;
    for (int a = threadIdx.x; a < n_acc; a += blockDim.x) {
        const int slot = ws.acc[(int64_t)b * p.k + a];
        const int id = p.cand[(int64_t)b * p.k + slot];
        const float* bx = db.boxes + (int64_t)id * 7;
        const float z = (float)((double)bx[2] - p.dz[(int64_t)b * p.k + slot]);
        rec[a] = make_box_rec(bx[0], bx[1], z, bx[3] + p.ew[0], bx[4] + p.ew[1], bx[5] + p.ew[2], bx[6], (double)1e-2f);
    }
    return n_acc;
}

__device__ __forceinline__ bool kept_point(const float* __restrict__ q, const BoxRec* rec, int n_acc) {
    const float x = q[0], y = q[1], z = q[2];
    for (int a = 0; a < n_acc; ++a)
        if (in_box_rec<false>(rec[a], x, y, z)) return false;
    return true;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ag_select_kernel(const int64_t* __restrict__ off, int64_t n_total, int64_t n_cap,
                                                        const float* __restrict__ boxes, const int64_t* __restrict__ boff,
                                                        int64_t m_total, Db db, Plan p, int64_t paste_cap, Ws ws) {
    __shared__ BevBox cb[AG_KMAX], eb[256];
    __shared__ int32_t grp[AG_KMAX], size[AG_KMAX], bad[AG_KMAX];
    __shared__ uint32_t ovl[AG_KMAX][AG_KWORDS];   // bit j of row k: candidate j of an earlier group overlaps k
    __shared__ int32_t status_sh, keep_sh;
    const int b = blockIdx.x, tid = threadIdx.x, K = p.k;
    if (tid == 0) { status_sh = 0; keep_sh = 0; }
    __syncthreads();
    const bool pts_ok = offsets_ok(off, b, n_total), box_ok = offsets_ok(boff, b, m_total);
    if (tid == 0) {
        int st = 0;
        if (!pts_ok || !box_ok) st |= ST_BAD_OFFSETS;
        else if (off[b + 1] - off[b] > n_cap) st |= ST_OVER_CAP;
        status_sh = st;
    }
    for (int k = tid; k < K; k += 256) {
        const int id = p.cand[(int64_t)b * K + k];
        int g = -1, n = 0;
        if (id >= 0 || id < -1) {
            if (object_ok(db, id)) {
                g = p.group[(int64_t)b * K + k];
                n = (int)(db.offsets[id + 1] - db.offsets[id]);
                cb[k] = make_box(db.boxes + (int64_t)id * 7);
            } else {
                atomicOr(&status_sh, ST_BAD_CAND);
            }
        }
        grp[k] = g;
        size[k] = n;
        bad[k] = 0;
        for (int w = 0; w < AG_KWORDS; ++w) ovl[k][w] = 0u;
    }
    __syncthreads();
    // groups must come in ascending order in the row: a later slot never belongs to an earlier group
    if (tid == 0) {
        int last = -1;
        for (int k = 0; k < K; ++k) {
            if (grp[k] < 0) continue;
            if (grp[k] < last) status_sh |= ST_BAD_CAND;
            last = grp[k];
        }
    }
    // existing boxes (every class), 256 at a time
    const int64_t bs = box_ok ? boff[b] : 0;
    const int m = box_ok ? (int)min(boff[b + 1] - bs, (int64_t)INT32_MAX) : 0;
    int keep = 0;
    for (int e0 = 0; e0 < m; e0 += 256) {
        const int ne = min(256, m - e0);
        __syncthreads();
        if (tid < ne) {
            const float* bx = boxes + (bs + e0 + tid) * 8;
            eb[tid] = make_box(bx);
            keep += (p.raw || bx[7] != 0.f) ? 1 : 0;
        }
        __syncthreads();
        for (int q = tid; q < K * ne; q += 256) {
            const int k = q / ne, e = q - k * ne;
            if (grp[k] >= 0 && iou_bev(cb[k], eb[e]) > 0.f) bad[k] = 1;
        }
    }
    if (keep) atomicAdd(&keep_sh, keep);
    // candidate pairs: the same group invalidates, an earlier group is remembered for the walk below
    for (int q = tid; q < K * K; q += 256) {
        const int k = q / K, j = q - k * K;
        if (j == k || grp[k] < 0 || grp[j] < 0 || grp[j] > grp[k]) continue;
        if (iou_bev(cb[k], cb[j]) > 0.f) {
            if (grp[j] == grp[k]) bad[k] = 1;
            else atomicOr(&ovl[k][j >> 5], 1u << (j & 31));
        }
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t accm[AG_KWORDS];
        for (int w = 0; w < AG_KWORDS; ++w) accm[w] = 0u;
        int n_acc = 0, n_paste = 0, st = status_sh;
        int32_t* acc = ws.acc + (int64_t)b * K;
        int32_t* pfx = ws.pfx + (int64_t)b * (K + 1);
        pfx[0] = 0;
        if (!(st & (ST_BAD_OFFSETS | ST_OVER_CAP))) {
            for (int k = 0; k < K; ++k) {
                if (grp[k] < 0 || bad[k]) continue;
                uint32_t hit = 0u;
                for (int w = 0; w < AG_KWORDS; ++w) hit |= ovl[k][w] & accm[w];
                if (hit) continue;
                accm[k >> 5] |= 1u << (k & 31);
                acc[n_acc++] = k;
                n_paste += size[k];
                pfx[n_acc] = n_paste;
            }
        }
        if (n_paste > paste_cap) { st |= ST_OVER_CAP; n_acc = n_paste = 0; }
        const int n_keep = (st & (ST_BAD_OFFSETS | ST_OVER_CAP)) ? 0 : keep_sh;
        if (n_keep + n_acc == 0) st |= ST_NO_BOX;
        ws.scene[b] = SceneRec{n_acc, n_paste, n_keep, st};
    }
}

__global__ __launch_bounds__(AG_TILE) void ag_count_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off, int c,
                                                           Db db, Plan p, int tiles, Ws ws) {
    __shared__ BoxRec rec[AG_KMAX];
    __shared__ int32_t wk[AG_WAVES];
    const int b = blockIdx.y, t = blockIdx.x;
    const SceneRec sr = ws.scene[b];
    const bool ok = !(sr.status & (ST_BAD_OFFSETS | ST_OVER_CAP));
    const int n_acc = stage_removal_boxes(db, p, ws, b, rec);
    __syncthreads();
    const int64_t s = ok ? off[b] : 0;
    const int n = ok ? (int)(off[b + 1] - s) : 0;
    const int i = t * AG_TILE + (int)threadIdx.x;
    const bool kept = i < n && kept_point(pts + (s + i) * (int64_t)c, rec, n_acc);
    const uint64_t bk = __ballot(kept);
    if (lane_id() == 0) wk[wave_id()] = __popcll(bk);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t sum = 0;
        for (int w = 0; w < AG_WAVES; ++w) sum += wk[w];
        ws.tile[(int64_t)b * tiles + t] = sum;
    }
}

// One workgroup for the batch: the scenes one after another, each scene's tiles scanned by 1024 threads.
__global__ __launch_bounds__(1024) void ag_scan_kernel(int batch, int tiles, Ws ws, int64_t out_cap, int64_t box_cap,
                                                       int64_t* __restrict__ out_off, int64_t* __restrict__ out_boff,
                                                       int32_t* __restrict__ info) {
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
        SceneRec sr = ws.scene[b];
        int64_t n_out = (int64_t)sr.n_paste + ps[1023];
        int64_t m_out = (int64_t)sr.n_keep_boxes + sr.n_acc;
        if (sr.status & (ST_BAD_OFFSETS | ST_OVER_CAP)) n_out = m_out = 0;
        if (run + n_out > out_cap || brun + m_out > box_cap) {
            sr.status |= ST_OVER_CAP;
            n_out = m_out = 0;
        }
        __syncthreads();
        if (u == 0) {
            out_off[b] = run;
            out_boff[b] = brun;
            if (sr.status & ST_OVER_CAP) ws.scene[b].status = sr.status;
            info[b * 4 + 0] = (int32_t)n_out;
            info[b * 4 + 1] = (int32_t)m_out;
            info[b * 4 + 2] = m_out ? sr.n_acc : 0;
            info[b * 4 + 3] = sr.status;
        }
        run += n_out;
        brun += m_out;
    }
    if (u == 0) {
        out_off[batch] = run;
        out_boff[batch] = brun;
    }
}

__global__ __launch_bounds__(AG_TILE) void ag_write_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off, int c,
                                                           const float* __restrict__ boxes, const int64_t* __restrict__ boff,
                                                           Db db, Plan p, int tiles, Ws ws, const int64_t* __restrict__ out_off,
                                                           const int64_t* __restrict__ out_boff, float* __restrict__ out,
                                                           float* __restrict__ out_boxes) {
    __shared__ BoxRec rec[AG_KMAX];
    __shared__ int32_t wk[AG_WAVES];
    __shared__ int32_t kept_sh;
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const SceneRec sr = ws.scene[b];
    const int64_t o0 = out_off[b];
    if (out_off[b + 1] == o0 && out_boff[b + 1] == out_boff[b]) return;   // nothing to write (or a flagged scene)
    const Xf xf = xf_of(p, b);
    const int K = p.k;
    if (t < tiles) {                                                       // kept scene points, stable
        const int n_acc = stage_removal_boxes(db, p, ws, b, rec);
        __syncthreads();
        const int64_t s = off[b];
        const int n = (int)(off[b + 1] - s);
        const int i = t * AG_TILE + tid;
        const float* q = pts + (s + i) * (int64_t)c;
        const bool kept = i < n && kept_point(q, rec, n_acc);
        const uint64_t bk = __ballot(kept);
        const int w = wave_id();
        if (lane_id() == 0) wk[w] = __popcll(bk);
        __syncthreads();
        if (!kept) return;
        int64_t pos = o0 + sr.n_paste + ws.tile[(int64_t)b * tiles + t] + rank_below(bk);
        for (int v = 0; v < w; ++v) pos += wk[v];
        float x = q[0], y = q[1], z = q[2];
        xf_point(xf, x, y, z);
        float* o = out + pos * c;
        o[0] = x; o[1] = y; o[2] = z;
        for (int f = 3; f < c; ++f) o[f] = q[f];
    } else if (t < (int)gridDim.x - 1) {                                  // pasted object points
        const int j = (t - tiles) * AG_TILE + tid;
        if (j >= sr.n_paste) return;
        const int32_t* pfx = ws.pfx + (int64_t)b * (K + 1);
        int lo = 0, hi = sr.n_acc;                                         // the last a with pfx[a] <= j
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (pfx[mid] <= j) lo = mid;
            else hi = mid;
        }
        const int slot = ws.acc[(int64_t)b * K + lo];
        const int id = p.cand[(int64_t)b * K + slot];
        const double dz = p.dz[(int64_t)b * K + slot];
        const double* ctr = db.centre + (int64_t)id * 3;
        const float* q = db.points + (db.offsets[id] + (j - pfx[lo])) * (int64_t)c;
        // obj_points[:, :3] += box3d_lidar[:3] (float64) then obj_points[:, 2] -= mv_height: double, rounded to float
        float x = (float)((double)q[0] + ctr[0]), y = (float)((double)q[1] + ctr[1]), z = (float)((double)q[2] + ctr[2]);
        z = (float)((double)z - dz);
        xf_point(xf, x, y, z);
        float* o = out + (o0 + j) * c;
        o[0] = x; o[1] = y; o[2] = z;
        for (int f = 3; f < c; ++f) o[f] = q[f];
    } else {                                                               // boxes: kept existing ones, then the accepted
        float* ob = out_boxes + out_boff[b] * 8;
        const int64_t bs = boff[b];
        const int m = (int)(boff[b + 1] - bs);
        if (tid == 0) kept_sh = 0;
        __syncthreads();
        for (int e0 = 0; e0 < m; e0 += AG_TILE) {
            const int e = e0 + tid;
            const float* bx = boxes + (bs + e) * 8;
            const bool keep = e < m && (p.raw || bx[7] != 0.f);
            const uint64_t bk = __ballot(keep);
            const int w = wave_id();
            if (lane_id() == 0) wk[w] = __popcll(bk);
            __syncthreads();
            int pos = kept_sh + rank_below(bk);
            for (int v = 0; v < w; ++v) pos += wk[v];
            if (keep) {
                float x = bx[0], y = bx[1], z = bx[2];
                xf_point(xf, x, y, z);
                float* o = ob + (int64_t)pos * 8;
                o[0] = x; o[1] = y; o[2] = z;
                o[3] = bx[3] * xf.sc; o[4] = bx[4] * xf.sc; o[5] = bx[5] * xf.sc;
                o[6] = heading_of(p, xf, bx[6]);
                o[7] = bx[7];
            }
            __syncthreads();
            if (tid == 0) for (int v = 0; v < AG_WAVES; ++v) kept_sh += wk[v];
            __syncthreads();
        }
        const int n_keep = kept_sh;
        for (int a = tid; a < sr.n_acc; a += AG_TILE) {
            const int slot = ws.acc[(int64_t)b * K + a];
            const int id = p.cand[(int64_t)b * K + slot];
            const float* bx = db.boxes + (int64_t)id * 7;
            float x = bx[0], y = bx[1], z = (float)((double)bx[2] - p.dz[(int64_t)b * K + slot]);
            xf_point(xf, x, y, z);
            float* o = ob + (int64_t)(n_keep + a) * 8;
            o[0] = x; o[1] = y; o[2] = z;
            o[3] = bx[3] * xf.sc; o[4] = bx[4] * xf.sc; o[5] = bx[5] * xf.sc;
            o[6] = heading_of(p, xf, bx[6]);
            o[7] = (float)db.cls[id];
        }
    }
}

int64_t al256(int64_t x) { return (x + 255) / 256 * 256; }
bool aug_sizes_ok(int batch, int64_t n_cap, int k) {
    return batch >= 0 && batch <= 65535 && n_cap >= 1 && n_cap <= (1 << 30) && k >= 0 && k <= AG_KMAX;
}
int64_t aug_tiles(int64_t n_cap) { return divup64(n_cap, AG_TILE); }

}  // namespace
}  // namespace pda

PDA_API int64_t pda_augment_workspace_bytes(int batch, int64_t n_cap, int k) {
    if (!pda::aug_sizes_ok(batch, n_cap, k)) return -1;
    return pda::al256((int64_t)batch * 16) + pda::al256((int64_t)batch * k * 4) + pda::al256((int64_t)batch * (k + 1) * 4) +
           pda::al256((int64_t)batch * pda::aug_tiles(n_cap) * 4);
}

// pda_augment (raw = 0) and its paste-only form pda_augment_paste (raw = 1: no flip / angle / scale)
static int augment_launch(const char* what, int raw, const float* points, const int64_t* offsets, int64_t n_total, int batch,
                        int c, int64_t n_cap, const float* boxes, const int64_t* box_offsets, int64_t m_total, const float* db_points,
                        const int64_t* db_offsets, int64_t db_n_points, const float* db_boxes, const double* db_centre,
                        const int32_t* db_class, int n_obj, const int32_t* cand, const int32_t* cand_group,
                        const double* cand_dz, int k, const int32_t* flip, const double* angle, const float* scale,
                        const float* remove_extra_width, int64_t paste_cap, float* out_points, int64_t out_cap,
                        int64_t* out_offsets, float* out_boxes, int64_t out_box_cap, int64_t* out_box_offsets, int32_t* info,
                        void* workspace, pda_stream_t stream) {
    PDA_REQUIRE(pda::aug_sizes_ok(batch, n_cap, k) && n_total >= 0 && c >= 3 && c <= 64 && m_total >= 0 && db_n_points >= 0 &&
                    n_obj >= 0 && paste_cap >= 0 && paste_cap <= (1 << 30) && out_cap >= 0 && out_box_cap >= 0,
                "%s: bad size: batch=%d n_total=%lld C=%d n_cap=%lld m_total=%lld db_points=%lld n_obj=%d K=%d "
                "paste_cap=%lld out_cap=%lld out_box_cap=%lld",
                what, batch, (long long)n_total, c, (long long)n_cap, (long long)m_total, (long long)db_n_points, n_obj, k,
                (long long)paste_cap, (long long)out_cap, (long long)out_box_cap);
    if (batch == 0) return PDA_OK;
    PDA_REQUIRE(offsets && box_offsets && out_offsets && out_box_offsets && info && workspace && remove_extra_width &&
                    (raw || (flip && angle && scale)) && (points || n_total == 0) && (boxes || m_total == 0) &&
                    (out_points || out_cap == 0) && (out_boxes || out_box_cap == 0) && (k == 0 || (cand && cand_group && cand_dz)) &&
                    (n_obj == 0 || (db_offsets && db_boxes && db_centre && db_class)) && (db_points || db_n_points == 0),
                "%s: null pointer", what);
    const int tiles = (int)pda::aug_tiles(n_cap);
    const int ptiles = (int)pda::divup64(paste_cap, pda::AG_TILE);
    char* w = (char*)workspace;
    pda::Ws ws;
    ws.scene = (pda::SceneRec*)w;
    w += pda::al256((int64_t)batch * 16);
    ws.acc = (int32_t*)w;
    w += pda::al256((int64_t)batch * k * 4);
    ws.pfx = (int32_t*)w;
    w += pda::al256((int64_t)batch * (k + 1) * 4);
    ws.tile = (int32_t*)w;
    const pda::Db db{db_points, db_offsets, db_boxes, db_centre, db_class, db_n_points, n_obj};
    const pda::Plan p{cand, cand_group, cand_dz, flip, angle, scale,
                      {remove_extra_width[0], remove_extra_width[1], remove_extra_width[2]}, k, raw};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pda::ag_select_kernel, dim3((unsigned)batch), dim3(256), 0, st, offsets, n_total, n_cap, boxes, box_offsets,
                       m_total, db, p, paste_cap, ws);
    hipLaunchKernelGGL(pda::ag_count_kernel, dim3((unsigned)tiles, (unsigned)batch), dim3(pda::AG_TILE), 0, st, points, offsets, c,
                       db, p, tiles, ws);
    hipLaunchKernelGGL(pda::ag_scan_kernel, dim3(1), dim3(1024), 0, st, batch, tiles, ws, out_cap, out_box_cap, out_offsets,
                       out_box_offsets, info);
    hipLaunchKernelGGL(pda::ag_write_kernel, dim3((unsigned)(tiles + ptiles + 1), (unsigned)batch), dim3(pda::AG_TILE), 0, st,
                       points, offsets, c, boxes, box_offsets, db, p, tiles, ws, out_offsets, out_box_offsets, out_points,
                       out_boxes);
    return pda::check_launch(what);
}

PDA_API int pda_augment(const float* points, const int64_t* offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                        const float* boxes, const int64_t* box_offsets, int64_t m_total, const float* db_points,
                        const int64_t* db_offsets, int64_t db_n_points, const float* db_boxes, const double* db_centre,
                        const int32_t* db_class, int n_obj, const int32_t* cand, const int32_t* cand_group,
                        const double* cand_dz, int k, const int32_t* flip, const double* angle, const float* scale,
                        const float* remove_extra_width, int64_t paste_cap, float* out_points, int64_t out_cap,
                        int64_t* out_offsets, float* out_boxes, int64_t out_box_cap, int64_t* out_box_offsets, int32_t* info,
                        void* workspace, pda_stream_t stream) {
    return augment_launch("pda_augment", 0, points, offsets, n_total, batch, c, n_cap, boxes, box_offsets, m_total, db_points,
                          db_offsets, db_n_points, db_boxes, db_centre, db_class, n_obj, cand, cand_group, cand_dz, k, flip,
                          angle, scale, remove_extra_width, paste_cap, out_points, out_cap, out_offsets, out_boxes, out_box_cap,
                          out_box_offsets, info, workspace, stream);
}

PDA_API int pda_augment_paste(const float* points, const int64_t* offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                              const float* boxes, const int64_t* box_offsets, int64_t m_total, const float* db_points,
                              const int64_t* db_offsets, int64_t db_n_points, const float* db_boxes, const double* db_centre,
                              const int32_t* db_class, int n_obj, const int32_t* cand, const int32_t* cand_group,
                              const double* cand_dz, int k, const float* remove_extra_width, int64_t paste_cap,
                              float* out_points, int64_t out_cap, int64_t* out_offsets, float* out_boxes, int64_t out_box_cap,
                              int64_t* out_box_offsets, int32_t* info, void* workspace, pda_stream_t stream) {
    return augment_launch("pda_augment_paste", 1, points, offsets, n_total, batch, c, n_cap, boxes, box_offsets, m_total,
                          db_points, db_offsets, db_n_points, db_boxes, db_centre, db_class, n_obj, cand, cand_group, cand_dz, k,
                          nullptr, nullptr, nullptr, remove_extra_width, paste_cap, out_points, out_cap, out_offsets, out_boxes,
                          out_box_cap, out_box_offsets, info, workspace, stream);
}
