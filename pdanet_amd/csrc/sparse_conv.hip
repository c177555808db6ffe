// sparse_conv.hip -- the feature kernels of the sparse 3D convolutions (include/pda_train.h, pda_spconv_gemm / _wgrad), over
// the neighbour maps of sparse_conv_index.hip.  float32 in, float32 accumulate on the matrix cores with the exact f32-input
// MFMA v_mfma_f32_16x16x4_f32: bit for bit an f32 fmaf chain, so integer-valued data below 2^24 comes out exact and nothing
// here rounds operands to bf16.
//
// sc_gemm       : out[i] = sum_t in[nbr[i][t]] . plane[t] (+ bias), a gather-GEMM.  A workgroup owns 64 consecutive output
//                 rows, a wave 16 of them with every output column in registers; per tap one ballot tells whether any of the
//                 wave's rows reads a neighbour, and a tap nobody reads costs nothing more.  The operand rows are gathered in
//                 the load (no gathered copy exists in memory), every output row is written once: no scatter, no atomics.
//                 Output rows come in key order, so the rows of a tile are spatial neighbours and their gathers hit the same
//                 input rows in cache.  The data gradient is the same kernel over nbr_in (for a submanifold convolution over
//                 nbr_out with the taps mirrored) and the transposed planes.
// sc_wgrad_part : dW_t = sum_i in[nbr[i][t]]^T . grad_out[i], one workgroup per (row block, tap), its partial product to the
//                 workspace; sc_wgrad_sum adds the row blocks in ascending order and writes the (C_out, T, C_in) layout.
// sc_bias_part / sc_bias_sum : the column sums of grad_out by the same two steps.
// No float atomics anywhere: two runs give the same bits.
// A plane is (T, Kp, Np) float32: K the reduction width and N the output width, both padded with zeros to a multiple of 16.
#include "pda_common.h"

namespace pda {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SC_THREADS = 256;
constexpr int SC_WAVE_ROWS = 16;
constexpr int SC_ROWS = SC_WAVE_ROWS * (SC_THREADS / PDA_WAVE);      // output rows of a workgroup
constexpr int SC_MAX_C = 128;
constexpr int SC_MAX_T = 125;
constexpr int SC_MAX_BLOCKS = 64;                                     // row blocks of the weight gradient
constexpr int64_t SC_MAX_ROWS = 1 << 30;

inline int pad16(int c) { return (c + 15) / 16 * 16; }

// lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; D[row 4 * (l >> 4) + reg][col l & 15].
template <int NB>
__global__ __launch_bounds__(SC_THREADS) void sc_gemm(const float* __restrict__ in, const int32_t* __restrict__ nbr,
                                                      const float* __restrict__ plane, const float* __restrict__ bias,
                                                      float* __restrict__ out, int n_rows, int n_src, int T, int flip, int K,
                                                      int Kp, int N) {
    const int lane = lane_id(), col = lane & 15, kq = lane >> 4;
    const int r0 = blockIdx.x * SC_ROWS + wave_id() * SC_WAVE_ROWS;
    if (r0 >= n_rows) return;                                         // wave-uniform, and the kernel has no barrier
    const int row = r0 + col;
    f32x4 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool vec = (K & 3) == 0;
    for (int t = 0; t < T; ++t) {
        int j = row < n_rows ? nbr[(int64_t)row * T + (flip ? T - 1 - t : t)] : -1;
        if (j >= n_src) j = -1;
        if (__ballot(j >= 0) == 0) continue;
        const float* src = in + (int64_t)(j < 0 ? 0 : j) * K;
        const float* wt = plane + (int64_t)t * Kp * (NB * 16) + col;
        for (int kc = 0; kc < Kp; kc += 16) {
            const int k0 = kc + 4 * kq;
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            if (j >= 0) {
                if (vec) {
                    if (k0 < K) {
                        const float4 v = load4(src + k0);
                        a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (k0 + e < K) a[e] = src[k0 + e];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float* wrow = wt + (int64_t)(k0 + e) * (NB * 16);
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], wrow[b * 16], acc[b], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int c = b * 16 + col;
        if (c >= N) continue;
        const float add = bias ? bias[c] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = r0 + 4 * kq + r;
            if (o < n_rows) out[(int64_t)o * N + c] = acc[b][r] + add;
        }
    }
}

// part[((t * nblocks + rb) * Kp + ci) * Np + co] = sum over the rows of block rb of in[nbr[i][t]][ci] * grad_out[i][co]; a wave
// takes the 16 x 16 blocks of the product in turn, four rows an MFMA.
__global__ __launch_bounds__(SC_THREADS) void sc_wgrad_part(const float* __restrict__ in, const float* __restrict__ go,
                                                            const int32_t* __restrict__ nbr, int n_out, int n_in, int T, int cin,
                                                            int cout, int Kp, int Np, int rows_per_block,
                                                            float* __restrict__ part) {
    const int lane = lane_id(), col = lane & 15, kq = lane >> 4;
    const int rb = blockIdx.x, t = blockIdx.y;
    const int r_beg = rb * rows_per_block, r_end = min(n_out, r_beg + rows_per_block);
    const int nbn = Np / 16, nblk = (Kp / 16) * nbn;
    float* dst = part + ((int64_t)t * gridDim.x + rb) * Kp * Np;
    for (int blk = wave_id(); blk < nblk; blk += SC_THREADS / PDA_WAVE) {
        const int m0 = (blk / nbn) * 16, c0 = (blk % nbn) * 16;
        const int ci = m0 + col, co = c0 + col;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int r = r_beg; r < r_end; r += 4) {
            const int rr = r + kq;
            int j = rr < r_end ? nbr[(int64_t)rr * T + t] : -1;
            if (j >= n_in) j = -1;
            if (__ballot(j >= 0) == 0) continue;
            const float a = (j >= 0 && ci < cin) ? in[(int64_t)j * cin + ci] : 0.f;
            const float b = (j >= 0 && co < cout) ? go[(int64_t)rr * cout + co] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(int64_t)(m0 + 4 * kq + r) * Np + co] = acc[r];
    }
}

__global__ __launch_bounds__(SC_THREADS) void sc_wgrad_sum(const float* __restrict__ part, int nblocks, int T, int cin, int cout,
                                                           int Kp, int Np, float* __restrict__ grad_w) {
    const int64_t id = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (id >= (int64_t)cout * T * cin) return;
    const int ci = (int)(id % cin), t = (int)((id / cin) % T), co = (int)(id / ((int64_t)cin * T));
    const float* p = part + ((int64_t)t * nblocks * Kp + ci) * Np + co;
    float s = 0.f;
    for (int b = 0; b < nblocks; ++b) s = s + p[(int64_t)b * Kp * Np];
    grad_w[id] = s;
}

__global__ __launch_bounds__(SC_MAX_C) void sc_bias_part(const float* __restrict__ go, int n_out, int cout, int rows_per_block,
                                                         float* __restrict__ bpart) {
    const int c = threadIdx.x, rb = blockIdx.x;
    if (c >= cout) return;
    const int r_end = min(n_out, (rb + 1) * rows_per_block);
    float s = 0.f;
    for (int r = rb * rows_per_block; r < r_end; ++r) s = s + go[(int64_t)r * cout + c];
    bpart[rb * cout + c] = s;
}

__global__ __launch_bounds__(SC_MAX_C) void sc_bias_sum(const float* __restrict__ bpart, int nblocks, int cout,
                                                        float* __restrict__ grad_bias) {
    const int c = threadIdx.x;
    if (c >= cout) return;
    float s = 0.f;
    for (int b = 0; b < nblocks; ++b) s = s + bpart[b * cout + c];
    grad_bias[c] = s;
}

bool channels_ok(int cin, int cout) { return cin >= 1 && cin <= SC_MAX_C && cout >= 16 && cout <= SC_MAX_C && cout % 16 == 0; }

int wgrad_blocks(int64_t n_out) {
    const int64_t b = divup64(n_out, 256);
    return (int)(b < 1 ? 1 : (b > SC_MAX_BLOCKS ? SC_MAX_BLOCKS : b));
}
int wgrad_rows(int64_t n_out) { return (int)(divup64(divup64(n_out, wgrad_blocks(n_out)), 4) * 4); }

}  // namespace
}  // namespace pda

#define SC_REQUIRE_CHANNELS(who)                                                                                              \
    PDA_REQUIRE(pda::channels_ok(cin, cout),                                                                                  \
                who ": unsupported channels: C_in=%d (1 .. %d), C_out=%d (a multiple of 16 up to %d)", cin, pda::SC_MAX_C,    \
                cout, pda::SC_MAX_C)

PDA_API int pda_spconv_gemm(const float* in, const int32_t* nbr, const float* plane, const float* bias, float* out,
                            int64_t n_rows, int64_t n_src, int taps, int cin, int cout, int transposed, int flip,
                            pda_stream_t stream) {
    PDA_REQUIRE(n_rows >= 0 && n_rows <= pda::SC_MAX_ROWS && n_src >= 0 && n_src <= pda::SC_MAX_ROWS && taps >= 1 &&
                    taps <= pda::SC_MAX_T && (transposed == 0 || transposed == 1) && (flip == 0 || flip == 1),
                "pda_spconv_gemm: bad size: rows=%lld source rows=%lld taps=%d transposed=%d flip=%d", (long long)n_rows,
                (long long)n_src, taps, transposed, flip);
    SC_REQUIRE_CHANNELS("pda_spconv_gemm");
    if (n_rows == 0) return PDA_OK;
    PDA_REQUIRE(nbr && plane && out && (in || n_src == 0), "pda_spconv_gemm: null pointer");
    const int K = transposed ? cout : cin, N = transposed ? cin : cout;
    const int Kp = pda::pad16(K), nb = pda::pad16(N) / 16;
    const dim3 grid((unsigned)pda::divup64(n_rows, pda::SC_ROWS)), block(pda::SC_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define SC_LAUNCH(NB)                                                                                                         \
    case NB:                                                                                                                  \
        hipLaunchKernelGGL(pda::sc_gemm<NB>, grid, block, 0, st, in, nbr, plane, bias, out, (int)n_rows, (int)n_src, taps, flip, K, \
                           Kp, N);                                                                                            \
        break
    switch (nb) {
        SC_LAUNCH(1); SC_LAUNCH(2); SC_LAUNCH(3); SC_LAUNCH(4); SC_LAUNCH(5); SC_LAUNCH(6); SC_LAUNCH(7); SC_LAUNCH(8);
    }
#undef SC_LAUNCH
    return pda::check_launch("pda_spconv_gemm");
}

PDA_API int64_t pda_spconv_wgrad_workspace_bytes(int64_t n_out, int taps, int cin, int cout) {
    if (n_out < 0 || n_out > pda::SC_MAX_ROWS || taps < 1 || taps > pda::SC_MAX_T || !pda::channels_ok(cin, cout)) return -1;
    const int64_t nb = pda::wgrad_blocks(n_out);
    return (nb * taps * pda::pad16(cin) * pda::pad16(cout) + nb * cout) * 4;
}

PDA_API int pda_spconv_wgrad(const float* in, const float* grad_out, const int32_t* nbr_out, int64_t n_out, int64_t n_in, int taps,
                             int cin, int cout, float* grad_weight, float* grad_bias, void* workspace, pda_stream_t stream) {
    PDA_REQUIRE(n_out >= 0 && n_out <= pda::SC_MAX_ROWS && n_in >= 0 && n_in <= pda::SC_MAX_ROWS && taps >= 1 &&
                    taps <= pda::SC_MAX_T,
                "pda_spconv_wgrad: bad size: rows=%lld source rows=%lld taps=%d", (long long)n_out, (long long)n_in, taps);
    SC_REQUIRE_CHANNELS("pda_spconv_wgrad");
    PDA_REQUIRE(grad_weight && workspace && (n_out == 0 || (grad_out && nbr_out && (in || n_in == 0))),
                "pda_spconv_wgrad: null pointer");
    const int nb = pda::wgrad_blocks(n_out), rows = pda::wgrad_rows(n_out), Kp = pda::pad16(cin), Np = pda::pad16(cout);
    float* part = (float*)workspace;
    float* bpart = part + (int64_t)nb * taps * Kp * Np;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pda::sc_wgrad_part, dim3((unsigned)nb, (unsigned)taps), dim3(pda::SC_THREADS), 0, st, in, grad_out, nbr_out,
                       (int)n_out, (int)n_in, taps, cin, cout, Kp, Np, rows, part);
    hipLaunchKernelGGL(pda::sc_wgrad_sum, dim3((unsigned)pda::divup64((int64_t)cout * taps * cin, pda::SC_THREADS)),
                       dim3(pda::SC_THREADS), 0, st, part, nb, taps, cin, cout, Kp, Np, grad_weight);
    if (grad_bias) {
        hipLaunchKernelGGL(pda::sc_bias_part, dim3((unsigned)nb), dim3(pda::SC_MAX_C), 0, st, grad_out, (int)n_out, cout, rows, bpart);
        hipLaunchKernelGGL(pda::sc_bias_sum, dim3(1), dim3(pda::SC_MAX_C), 0, st, bpart, nb, cout, grad_bias);
    }
    return pda::check_launch("pda_spconv_wgrad");
}
