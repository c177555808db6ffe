/* pda_train.h -- C ABI of the "next rows" around the sampling/grouping path:
 * the train-step arithmetic and the target-assignment / post-processing kernels.  Same library
 * (libpda_pointnet2.so), same conventions as pda_pointnet2.h: device pointers, explicit stream,
 * status return + pda_last_error(), nothing allocated, no torch types.
 */
#ifndef PDA_TRAIN_H
#define PDA_TRAIN_H
#include "pda_pointnet2.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- adam_onecycle step (tools/train_utils/optimization/fastai_optim.py:138-156 OptimWrapper.step
 * with true_wd=True, bn_wd=True, wrapping torch.optim.Adam(betas=(mom, 0.99)); preceded by
 * clip_grad_norm_ in tools/train_utils/train_utils.py:56) on FLAT fp32 buffers: all trained
 * parameters, their gradients and both Adam moments each live in one contiguous allocation.
 *
 * pda_grad_norm: norm_out[0] = sqrt(sum g^2) in a fixed two-stage order (deterministic);
 *   scratch holds 1024 floats.
 * pda_adam_onecycle_step, per element:
 *   g' = g * min(1, max_norm / (total_norm + 1e-6))         (total_norm == NULL: no clipping)
 *   p  = p * (1 - wd * lr)                                   (decoupled decay, before Adam)
 *   m += (g' - m) * (1 - beta1);  v = v * beta2 + (1 - beta2) * g' * g'
 *   p -= (lr / (1 - beta1^step)) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * `step` is the 1-based Adam step count.  g is not modified. */
int pda_grad_norm(const float *g, int64_t n, float *norm_out, float *scratch1024, pda_stream_t stream);
int pda_adam_onecycle_step(float *p, const float *g, float *m, float *v, int64_t n, float lr,
                           float beta1, float beta2, float eps, float wd, int step,
                           const float *total_norm, float max_norm, pda_stream_t stream);

/* ---- training-mode BatchNorm + ReLU over the last dimension (MI355X extension) ---------------------
 * The point-major form of the reference's Conv1x1 -> BatchNorm -> ReLU stacks (pointnet2_modules.py:
 * 1605-1611, :628-671): x (rows, C) -> y = relu((x - mean_c) / sqrt(var_c + eps) * gamma_c + beta_c) with
 * batch statistics over the rows (biased variance), running statistics updated as nn.BatchNorm does
 * (momentum, unbiased variance; pass NULL for both to skip).  mean_invstd (2, C) is written for the
 * backward pass.  Backward: grad_x (rows, C), grad_gamma (C), grad_beta (C) are fully written.
 * C: power of two in [4, 1024]; anything else returns PDA_ERR_INVALID_ARGUMENT (callers keep the
 * framework's batch_norm + relu).  scratch: pda_bn_relu_scratch_bytes(C) bytes, 16-byte aligned. */
int64_t pda_bn_relu_scratch_bytes(int c);
int pda_bn_relu_fwd(const float *x, const float *gamma, const float *beta, float *running_mean,
                    float *running_var, float *y, float *mean_invstd, void *scratch, int64_t rows, int c,
                    float eps, float momentum, pda_stream_t stream);
int pda_bn_relu_bwd(const float *x, const float *grad_y, const float *gamma, const float *beta,
                    const float *mean_invstd, float *grad_x, float *grad_gamma, float *grad_beta,
                    void *scratch, int64_t rows, int c, pda_stream_t stream);
/* The counted form, for padded sparse tensors: `rows` is a capacity that sizes every grid, and the rows
 * that count are [0, *count), a device word clipped to [0, rows].  The same arithmetic as above over the live rows.  Dead rows
 * of x and grad_y are never read; dead rows of y and grad_x are written as exact zeros.  relu == 0: BatchNorm alone.
 * training == 0: normalise with the running statistics (required then), which are not updated.  In training mode *count < 2
 * ORs 8 into *status (torch would have raised): one row gives variance 0, no row leaves the running statistics alone.
 * rows == 0 is PDA_OK.  The same (live rows, capacity) gives the same bits from run to run. */
int pda_bn_relu_fwd_counted(const float *x, const float *gamma, const float *beta, float *running_mean, float *running_var,
                            float *y, float *mean_invstd, void *scratch, int64_t rows, int c, float eps, float momentum,
                            const int32_t *count, int32_t *status, int relu, int training, pda_stream_t stream);
int pda_bn_relu_bwd_counted(const float *x, const float *grad_y, const float *gamma, const float *beta,
                            const float *mean_invstd, float *grad_x, float *grad_gamma, float *grad_beta, void *scratch,
                            int64_t rows, int c, const int32_t *count, int relu, int training, pda_stream_t stream);
/* The residual tail of a sparse basic block in the counted form: y = max((xhat * gamma + beta) + identity, 0) over the live
 * rows [0, *count) of x, identity (cap, C).  Statistics, running buffers, *status and the C contract are those of
 * pda_bn_relu_fwd_counted; the BatchNorm value, the sum and the maximum round one after the other, so y has the bits of
 * pda_bn_relu_fwd_counted(relu = 0) followed by an addition and a ReLU.  Backward: y is the saved output and the ReLU mask is
 * y > 0; grad_identity (cap, C) is the masked gradient, grad_x its BatchNorm gradient, both written in one pass.  Dead rows of
 * x, identity, y and grad_y are never read; dead rows of y, grad_x and grad_identity are exact zeros.  cap == 0 is PDA_OK. */
int pda_bn_add_relu_fwd_counted(const float *x, const float *identity, const float *gamma, const float *beta,
                                float *running_mean, float *running_var, float *y, float *mean_invstd, void *scratch,
                                int64_t cap, int c, float eps, float momentum, const int32_t *count, int32_t *status,
                                int training, pda_stream_t stream);
int pda_bn_add_relu_bwd_counted(const float *x, const float *y, const float *grad_y, const float *gamma, const float *beta,
                                const float *mean_invstd, float *grad_x, float *grad_identity, float *grad_gamma,
                                float *grad_beta, void *scratch, int64_t cap, int c, const int32_t *count, int training,
                                pda_stream_t stream);
/* The reduction half of pda_bn_relu_bwd alone: grad_gamma, grad_beta and sums (2, C) = the per-channel means of the masked
 * gradient and of its product with the normalised input, for a consumer that forms grad_x itself (pda_sa_point_grad_bn). */
int pda_bn_relu_bwd_reduce(const float *x, const float *grad_y, const float *gamma, const float *beta,
                           const float *mean_invstd, float *grad_gamma, float *grad_beta, float *sums, void *scratch,
                           int64_t rows, int c, pda_stream_t stream);
/* Dense-bf16 mode variants (same kernels and fp32 / double arithmetic): x may be the bf16 output of a GEMM, y may be
 * written as bf16 (when it only feeds the next GEMM), grad_y may be bf16; grad_x has the element type of x. */
int pda_bn_relu_fwd_mixed(const void *x, int x_is_bf16, const float *gamma, const float *beta, float *running_mean,
                          float *running_var, void *y, int y_is_bf16, float *mean_invstd, void *scratch,
                          int64_t rows, int c, float eps, float momentum, pda_stream_t stream);
int pda_bn_relu_bwd_mixed(const void *x, int x_is_bf16, const void *grad_y, int grad_y_is_bf16, const float *gamma,
                          const float *beta, const float *mean_invstd, void *grad_x, float *grad_gamma,
                          float *grad_beta, void *scratch, int64_t rows, int c, pda_stream_t stream);
/* The last [BN -> ReLU] of a set-abstraction MLP together with the max-pool over the group's samples that follows it
 * (pointnet2_modules.py:1657-1670): x (groups*ns, C), row = group*ns + sample (fp32, or bf16 when x_is_bf16) ->
 * out (groups, C) = max over the ns rows of relu(bn(x)), arg (groups, C) uint8 = first row attaining it; the (rows, C)
 * activation is never written.  Backward takes grad_out (groups, C) and arg: the dense (rows, C) gradient is generated on
 * the fly inside the two BN-backward passes, never stored.  grad_x has the element type of x.  ns <= 255. */
int pda_bn_relu_max_pool_fwd(const void *x, int x_is_bf16, const float *gamma, const float *beta, float *running_mean,
                             float *running_var, float *out, uint8_t *arg, float *mean_invstd, void *scratch,
                             int64_t groups, int ns, int c, float eps, float momentum, pda_stream_t stream);
int pda_bn_relu_max_pool_bwd(const void *x, int x_is_bf16, const float *grad_out, const uint8_t *arg,
                             const float *gamma, const float *beta, const float *mean_invstd, void *grad_x,
                             float *grad_gamma, float *grad_beta, void *scratch, int64_t groups, int ns, int c,
                             pda_stream_t stream);

/* ---- LayerNorm over the last dimension with optional fused residual add (MI355X extension) ----------
 * nn.LayerNorm(D) of TransformerEncoderLayerPreNorm (PointFormer.py:17-18,29,33): x (rows, D) [+ residual
 * (rows, D), the sum also written to sum_out] -> y = (s - mean) / sqrt(var + eps) * gamma + beta per row
 * (biased variance); mean_rstd (rows, 2) kept for the backward pass, whose x argument is the normalised
 * tensor (x, or sum_out when a residual was added); grad_y2 (may be NULL) is a second incoming gradient
 * added to grad_y on the fly.  grad_x / grad_gamma / grad_beta are fully written.
 * D in {256, 512, 1024}.  scratch: pda_layer_norm_scratch_bytes(D) bytes. */
int64_t pda_layer_norm_scratch_bytes(int d);
int pda_layer_norm_fwd(const float *x, const float *residual, const float *gamma, const float *beta,
                       float *sum_out, float *y, float *mean_rstd, int64_t rows, int d, float eps,
                       pda_stream_t stream);
int pda_layer_norm_bwd(const float *x, const float *grad_y, const float *grad_y2, const float *gamma,
                       const float *mean_rstd, float *grad_x, float *grad_gamma, float *grad_beta,
                       void *scratch, int64_t rows, int d, pda_stream_t stream);
/* Dense-bf16 mode variants (same kernels, same fp32 arithmetic; bf16 = raw bit patterns, rounded to nearest even on the
 * store): x may be the bf16 output of a GEMM (x_is_bf16), y (fp32) and y_bf16 (a copy for the next bf16 GEMM) are each
 * optional (at least one); grad_y2 may be bf16; grad_x_bf16 (may be NULL) receives a bf16 copy of grad_x. */
int pda_layer_norm_fwd_mixed(const void *x, int x_is_bf16, const float *residual, const float *gamma,
                             const float *beta, float *sum_out, float *y, uint16_t *y_bf16, float *mean_rstd,
                             int64_t rows, int d, float eps, pda_stream_t stream);
int pda_layer_norm_bwd_mixed(const float *x, const float *grad_y, const void *grad_y2, int grad_y2_is_bf16,
                             const float *gamma, const float *mean_rstd, float *grad_x, uint16_t *grad_x_bf16,
                             float *grad_gamma, float *grad_beta, void *scratch, int64_t rows, int d,
                             pda_stream_t stream);

/* ---- weight / bias gradient of a linear layer over a long token axis (MI355X extension) -------------
 * The backward GEMMs of the point-major 1x1 convolutions and transformer projections: x (tokens, in),
 * grad_out (tokens, out), both row-major -> grad_weight (out, in) = grad_out^T x (the layout of
 * nn.Linear.weight / Conv.weight.flatten(1)) and, when grad_bias != NULL, grad_bias (out) = column sums
 * of grad_out.  Split over the token axis with a fixed-order second stage (deterministic).
 * in, out: multiples of 4.  scratch: pda_linear_wgrad_scratch_bytes(tokens, in, out) bytes.
 * pda_linear_wgrad_form: which kernel a call of this shape runs -- 0 the f32-MFMA split-K form, 1 the streaming form of
 * narrow layers (in, out <= 64), 2 the split-bf16 form (in, out multiples of 256, tokens * in * out >= 2e9). */
int64_t pda_linear_wgrad_scratch_bytes(int64_t tokens, int in_features, int out_features);
int pda_linear_wgrad_form(int64_t tokens, int in_features, int out_features);
int pda_linear_wgrad(const float *x, const float *grad_out, float *grad_weight, float *grad_bias,
                     void *scratch, int64_t tokens, int in_features, int out_features, pda_stream_t stream);
/* The same with x = the PRE-BatchNorm tensor of the layer: the weight gradient is taken against relu(bn(x)) formed in the
 * operand load (x_mean_invstd (2, in) = mean | invstd of the batch, x_gamma, x_beta (in)); the layer's activation need not
 * exist in memory.  Only shapes with pda_linear_wgrad_form == 2; otherwise PDA_ERR_UNSUPPORTED. */
int pda_linear_wgrad_bn(const float *x, const float *grad_out, float *grad_weight, float *grad_bias, void *scratch,
                        int64_t tokens, int in_features, int out_features, const float *x_mean_invstd,
                        const float *x_gamma, const float *x_beta, pda_stream_t stream);

/* ---- parameter gradients finished later: first stages alone, one grouped second stage (MI355X extension) -------
 * The second stage of pda_linear_wgrad (the fixed-order sum of the split-K partials) and of pda_layer_norm_bwd (the sum
 * of the per-block dgamma / dbeta partials) is a few workgroups of load latency, and nothing but the optimizer reads what
 * it writes.  A caller may therefore run the first stages alone and finish many gradients with one launch:
 * pda_linear_wgrad_partials / pda_linear_wgrad_bn_partials: the first stage of pda_linear_wgrad / pda_linear_wgrad_bn on
 * the same operands; scratch (pda_linear_wgrad_scratch_bytes) keeps part_w [S][out * in] and, with want_bias, part_b
 * [S][out] from float offset S * out * in; *slices = S (written on the host).
 * pda_layer_norm_bwd_partials: pda_layer_norm_bwd[_mixed] without its last launch: grad_x [and grad_x_bf16] are written,
 * scratch (pda_layer_norm_scratch_bytes) keeps the [nblocks][2][d] partials, *nblocks is written on the host.
 * pda_param_grad_reduce_grouped: n >= 1 entries (a host array, passed on as kernel arguments: no allocation, no copy, no
 * synchronisation; capturable; 48 entries per launch, more entries take more launches), each finished by the workgroups
 * and the order of additions of its per-problem kernel -- the same bits.
 *   kind 0, weight gradient: part = part_w, part_bias = part_b, count = S, nm = out * in, n = out, cols = in;
 *     dst (out rows of `cols` floats, `ld` >= cols floats apart: ld > cols writes a column block of a wider matrix),
 *     dst_bias (out) or NULL;
 *   kind 1, LayerNorm: part = the partials, count = nblocks, n = d, dst = grad_gamma, dst_bias = grad_beta (both d).
 * The partials must stay untouched until the grouped launch has run (stream order). */
typedef struct pda_param_grad_entry {
    int32_t kind, count;
    const float *part, *part_bias;
    float *dst, *dst_bias;
    int64_t nm;
    int32_t n, cols;
    int64_t ld;
} pda_param_grad_entry_t;
int pda_linear_wgrad_partials(const float *x, const float *grad_out, void *scratch, int want_bias, int64_t tokens,
                              int in_features, int out_features, int *slices, pda_stream_t stream);
int pda_linear_wgrad_bn_partials(const float *x, const float *grad_out, void *scratch, int64_t tokens, int in_features,
                                 int out_features, const float *x_mean_invstd, const float *x_gamma,
                                 const float *x_beta, int *slices, pda_stream_t stream);
int pda_layer_norm_bwd_partials(const float *x, const float *grad_y, const void *grad_y2, int grad_y2_is_bf16,
                                const float *gamma, const float *mean_rstd, float *grad_x, uint16_t *grad_x_bf16,
                                void *scratch, int64_t rows, int d, int *nblocks, pda_stream_t stream);
int pda_param_grad_reduce_grouped(const pda_param_grad_entry_t *entries, int n, pda_stream_t stream);

/* ---- a [conv1x1 -> BatchNorm(batch statistics) -> ReLU] chain with the BatchNorm passes folded into the contractions
 * (MI355X extension; the group MLP of pointnet2_modules.py:1657-1662 in training).
 * pda_gemm_split_bn: y (tokens, n_out) = X' W^T on the 256 x 256 tile split-bf16 kernel (wf = pda_linear_split_pack planes,
 * K a multiple of 32 <= 1024), where X' = x, or relu(bn(x)) when in_mean_invstd (2, K) / in_gamma / in_beta (K) are given.
 * stats_mode 1: partial [pda_gemm_split_bn_tiles(tokens)][2][n_out] doubles = per-column sum and sum of squares of y over each
 * tile of 256 tokens (the statistics pass of the BatchNorm behind this contraction; finish with pda_bn_finalize_fwd).
 * Fixed summation order. */
int64_t pda_gemm_split_bn_tiles(int64_t tokens);
int pda_gemm_split_bn(const float *x, const void *wf, float *y, int64_t tokens, int k, int n_out,
                      const float *in_mean_invstd, const float *in_gamma, const float *in_beta, int stats_mode,
                      double *partial, pda_stream_t stream);
/* Inference: out (tokens / ns, n_out) = max over every group of ns consecutive token rows of relu?(x W^T + bias) -- the last layer
 * of an SA scale with the max over nsample in the epilogue; the (tokens, n_out) tensor is never written.  ns in {16, 32, 64},
 * tokens a multiple of ns, K a multiple of 32.  Same arithmetic as pda_gemm_split followed by the max. */
int pda_gemm_split_maxpool(const float *x, const void *wf, const float *bias, float *out, int64_t tokens, int k, int n_out,
                           int ns, int relu, pda_stream_t stream);
/* Inference: the first two layers of a wide SA scale in one launch.  y (b*m*ns, n_out) = relu?(A W2^T + bias2) with
 * A[token] = relu(point_rows[idx[token]] + W1[:, 0:3] (xyz[idx[token]] - new_xyz[group]) + bias1) -- what pda_sa_point_gather would
 * write -- formed in the operand load.  point_rows (b*n, K): the per-point projection of the features by W1[:, 3:]; w1 (K, ldw1);
 * wf: pda_linear_split_pack planes of W2 (n_out, K).  K a multiple of 32 <= 1024. */
int pda_gemm_split_gather(const float *point_rows, const float *xyz, const float *new_xyz, const int32_t *idx,
                          const float *w1, int ldw1, const float *bias1, const void *wf, const float *bias2, float *y,
                          int b, int n, int m, int ns, int k, int n_out, int relu, pda_stream_t stream);
/* The passes of pda_bn_relu_fwd / pda_bn_relu_max_pool_fwd one at a time.  pda_bn_stats_fwd: statistics of x only
 * (mean_invstd (2, C), running statistics updated); scratch: pda_bn_relu_scratch_bytes(c).  pda_bn_finalize_fwd: the same
 * from `nblocks` rows of per-block sums [nblocks][2][C] (count = the number of rows they cover).
 * pda_bn_relu_max_pool_apply: normalise + ReLU + max over ns with given statistics. */
int pda_bn_stats_fwd(const float *x, float *running_mean, float *running_var, float *mean_invstd, void *scratch,
                     int64_t rows, int c, float eps, float momentum, pda_stream_t stream);
int pda_bn_finalize_fwd(const double *partial, int nblocks, int c, int64_t count, float eps, float momentum,
                        float *mean_invstd, float *running_mean, float *running_var, pda_stream_t stream);
int pda_bn_relu_max_pool_apply(const float *x, const float *gamma, const float *beta, const float *mean_invstd,
                               float *out, uint8_t *arg, int64_t groups, int ns, int c, pda_stream_t stream);

/* Dense-bf16 mode: the bias gradient alone, column sums of the bf16 gradient g (rows, cols) -> out (cols) fp32 (fixed
 * summation order).  cols: multiple of 8, <= 2048; scratch: pda_colsum_scratch_bytes(cols) bytes. */
int64_t pda_colsum_scratch_bytes(int cols);
int pda_colsum_bf16(const uint16_t *g, float *out, void *scratch, int64_t rows, int cols, pda_stream_t stream);

/* Token assembly of a PDA scale (MI355X extension; pointnet2_modules.py:879-922), point-major:
 * out (B,M,ns,4C) = [rppe (B,M,ns,C) | f * dscale | f | glob (B,M,C) broadcast over ns] with f = feats (B,N,C)
 * gathered by idx (B,M,ns) and dscale (B,M,ns) the density score.  The gradient entry writes grad_rppe,
 * grad_dscale and grad_glob fully and ADDS into grad_feats (B,N,C), which the caller zero-fills.
 * C in {16, 32, 64, 128, 256}. */
int pda_assemble_tokens(const float *rppe, const float *dscale, const float *feats, const int32_t *idx,
                        const float *glob, float *out, int b, int n, int m, int nsample, int c,
                        pda_stream_t stream);
int pda_assemble_tokens_grad(const float *grad_out, const float *dscale, const float *feats, const int32_t *idx,
                             float *grad_rppe, float *grad_dscale, float *grad_feats, float *grad_glob,
                             int b, int n, int m, int nsample, int c, pda_stream_t stream);

/* Residual add + max-pool over the tokens of a group (MI355X extension; pointnet2_modules.py:929-931 on the
 * encoder layer's output): a, b (groups, seq, D) -> out (groups, D) = max over seq of a + b, arg (groups, D)
 * uint8 = token of the first maximum; pda_max_pool_scatter writes the dense (groups, seq, D) gradient
 * (grad_out routed to the arg-max token, zeros elsewhere).  seq <= 255, D multiple of 4. */
int pda_add_max_pool(const float *a, const float *b, float *out, uint8_t *arg, int64_t groups, int seq, int d,
                     pda_stream_t stream);
int pda_max_pool_scatter(const float *grad_out, const uint8_t *arg, float *grad_x, int64_t groups, int seq,
                         int d, pda_stream_t stream);
/* Dense-bf16 mode: b is the bf16 output of a GEMM; the scatter also writes a bf16 copy of the gradient. */
int pda_add_max_pool_bf16(const float *a, const uint16_t *b, float *out, uint8_t *arg, int64_t groups, int seq,
                          int d, pda_stream_t stream);
int pda_max_pool_scatter_bf16(const float *grad_out, const uint8_t *arg, float *grad_x, uint16_t *grad_x_bf16,
                              int64_t groups, int seq, int d, pda_stream_t stream);

/* Multiplicity-weighted training-mode BatchNorm + ReLU (rows stand for row_weight[r] identical rows of a dense tensor of
 * `count` rows): same results as pda_bn_relu_fwd/bwd on the dense tensor, with grad_y / grad_x the SUMS over the copies. */
int pda_bn_relu_fwd_weighted(const float *x, const float *gamma, const float *beta, float *running_mean,
                             float *running_var, float *y, float *mean_invstd, void *scratch, int64_t rows, int c,
                             float eps, float momentum, const float *row_weight, int64_t count, pda_stream_t stream);
int pda_bn_relu_bwd_weighted(const float *x, const float *grad_y, const float *gamma, const float *beta,
                             const float *mean_invstd, float *grad_x, float *grad_gamma, float *grad_beta,
                             void *scratch, int64_t rows, int c, const float *row_weight, int64_t count,
                             pda_stream_t stream);

/* ---- unique-token ("ragged") execution of a PDA scale (MI355X extension; csrc/ragged.hip) -----------------
 * ball_query pads a short neighbour list with repeats of its first entry (ball_query_gpu.cu:35-41), and the PDA
 * layer runs its transformer encoder over all nsample tokens of every centre (pointnet2_modules.py:924-931).  A
 * repeated neighbour is an identical token, so the encoder is evaluated on the DISTINCT tokens only: compact row
 * u in [off[g], off[g] + cnt[g]) is slot u - off[g] of group g.  Same results as the dense form in exact arithmetic
 * (key 0 of a group enters the softmax with weight nsample - cnt + 1; the max over a group ignores repeats; a
 * compact token receives the summed gradient of its copies).
 * pda_ragged_plan: idx (groups, nsample) -> cnt (groups), off (groups + 1; off[groups] = U = number of distinct
 *   tokens), rowmap (>= U; compact row -> dense row g * nsample + s), row_weight (>= U, optional: the multiplicity of
 *   each compact token, nsample - cnt + 1 for slot 0 and 1 otherwise).  No synchronisation: the caller reads U.
 * rppe_compact != 0: the position-encoding rows (and their gradient) are compact (U, C) as well -- the position MLP
 *   ran on the distinct tokens with pda_bn_relu_{fwd,bwd}_weighted (statistics of the dense tensor from weighted sums;
 *   a compact row's gradient is the sum over its copies).
 * pda_assemble_tokens_ragged(_grad): pda_assemble_tokens writing / reading compact rows (out (U, 4C)); the grid
 *   covers max_tokens >= U rows and reads U on the device.  The gradient entry writes the DENSE grad_rppe /
 *   grad_dscale (zero at the repeat slots) and grad_glob, and ADDS into grad_feats (zero-filled by the caller);
 *   with rowmap (and max_tokens >= U) its per-token part runs over (token, column) threads, with rowmap NULL one
 *   thread walks the tokens of a centre (same results; grad_feats is a float-atomic sum either way).
 * pda_add_max_pool_ragged / pda_max_pool_scatter_ragged: the add + max-pool tail on compact rows; arg = slot.
 * pda_group_attention_ragged_fwd/bwd (include/pda_pointnet2.h layout with compact rows): qkv (U, 3, H, hd),
 *   out / grad_out (U, H * hd), lse (groups, H, seq).  tokens = U (the caller has read it to size qkv): one wave
 *   packs the distinct tokens of several consecutive groups into 32-row tiles, and U / groups decides how many
 *   groups a wave takes (a wrong value costs speed, never results). */
int pda_ragged_plan(const int32_t *idx, int32_t *cnt, int32_t *off, int32_t *rowmap, float *row_weight, int64_t groups,
                    int nsample, pda_stream_t stream);
int pda_assemble_tokens_ragged(const float *rppe, const float *dscale, const float *feats, const int32_t *idx,
                               const float *glob, const int32_t *rowmap, const int32_t *off, float *out,
                               int64_t max_tokens, int b, int n, int m, int nsample, int c, int rppe_compact,
                               pda_stream_t stream);
int pda_assemble_tokens_ragged_grad(const float *grad_out, const float *dscale, const float *feats,
                                    const int32_t *idx, const int32_t *cnt, const int32_t *off, const int32_t *rowmap,
                                    float *grad_rppe, float *grad_dscale, float *grad_feats, float *grad_glob,
                                    int64_t max_tokens, int b, int n, int m, int nsample, int c, int rppe_compact,
                                    pda_stream_t stream);
int pda_add_max_pool_ragged(const float *a, const float *b, const int32_t *cnt, const int32_t *off, float *out,
                            uint8_t *arg, int64_t groups, int d, pda_stream_t stream);
int pda_max_pool_scatter_ragged(const float *grad_out, const uint8_t *arg, const int32_t *rowmap,
                                const int32_t *off, float *grad_x, int64_t max_tokens, int64_t groups, int nsample,
                                int d, pda_stream_t stream);
int pda_group_attention_ragged_fwd(const float *qkv, const int32_t *cnt, const int32_t *off, float *out, float *lse,
                                   int64_t tokens, int64_t num_groups, int seq, int heads, int head_dim,
                                   pda_stream_t stream);
int pda_group_attention_ragged_bwd(const float *qkv, const float *grad_out, const float *lse, const int32_t *cnt,
                                   const int32_t *off, float *grad_qkv, int64_t tokens, int64_t num_groups, int seq,
                                   int heads, int head_dim, pda_stream_t stream);

/* ---- DensityNet in training mode (MI355X extension) ----------------------------------------------
 * pointnet2_modules.py:958-981: y = relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x)))))))) with 1x1 convs
 * 1 -> 16 -> 8 -> 1 (with bias), batch statistics over the n tokens; x, y (n) fp32.
 * params (pda_densitynet_param_count() = 227 floats): w1[16] b1[16] gamma1[16] beta1[16] W2[8][16] b2[8]
 * gamma2[8] beta2[8] w3[8] b3 gamma3 beta3; grad_params has the same layout.  stats (46 floats) carries the
 * batch statistics to the backward pass; running_mean/var k (sizes 16, 8, 1) are updated like nn.BatchNorm
 * (all six NULL: skip).  The input receives no gradient (it is a function of coordinates only).
 * scratch: pda_densitynet_scratch_bytes() bytes. */
int pda_densitynet_param_count(void);
int64_t pda_densitynet_scratch_bytes(void);
int pda_densitynet_fwd(const float *x, const float *params, float *y, float *stats, void *scratch,
                       float *running_mean1, float *running_var1, float *running_mean2, float *running_var2,
                       float *running_mean3, float *running_var3, int64_t n, float eps, float momentum,
                       pda_stream_t stream);
int pda_densitynet_bwd(const float *x, const float *grad_y, const float *params, const float *stats,
                       float *grad_params, void *scratch, int64_t n, float eps, pda_stream_t stream);
/* The same on the DISTINCT slots of padded neighbour lists (pda_ragged_plan above): x, y, grad_y keep the dense
 * (groups, nsample) layout, n = groups * nsample, but only the *n_unique slots rowmap[0..) are evaluated, slot 0 of a
 * group standing for its row_weight = nsample - cnt + 1 identical tokens (ball_query's repeats, slots cnt..nsample-1,
 * hold the same x).  n_unique is DEVICE memory (off + groups of the plan): no host read.  Batch statistics, running
 * statistics and parameter gradients are those of the n dense tokens; forward writes every slot of y (a group's
 * repeats together with its slot 0); backward takes the gradient of a distinct slot as the sum over its copies.
 * Results equal pda_densitynet_fwd / _bwd up to the order of the floating-point additions. */
int pda_densitynet_fwd_unique(const float *x, const float *params, float *y, float *stats, void *scratch,
                              float *running_mean1, float *running_var1, float *running_mean2, float *running_var2,
                              float *running_mean3, float *running_var3, int64_t n, const int32_t *rowmap,
                              const float *row_weight, const int32_t *n_unique, int nsample, float eps, float momentum,
                              pda_stream_t stream);
int pda_densitynet_bwd_unique(const float *x, const float *grad_y, const float *params, const float *stats,
                              float *grad_params, void *scratch, int64_t n, const int32_t *rowmap,
                              const float *row_weight, const int32_t *n_unique, int nsample, float eps,
                              pda_stream_t stream);
/* Several independent DensityNet problems in ONE set of launches (the scales of a PDA layer: each of the nine passes is
 * ~10 us of dependency latency on <= 128 workgroups, so two problems per launch cost what one does).  Per problem the
 * arguments of the entries above; rowmap / row_weight / n_unique all NULL: every token (pda_densitynet_fwd), else the
 * distinct slots (pda_densitynet_fwd_unique).  Forward reads x, params, writes y, stats, running (all six or none);
 * backward reads x, grad_y, params, stats, writes grad_params.  scratch: pda_densitynet_scratch_bytes() each. */
#define PDA_DENSITYNET_MAX_SCALES 4
typedef struct pda_densitynet_scale {
    const float *x, *grad_y, *params;
    float *y, *stats;
    void *scratch;
    float *running[6]; /* mean1, var1, mean2, var2, mean3, var3 */
    float *grad_params;
    int64_t n;
    const int32_t *rowmap;
    const float *row_weight;
    const int32_t *n_unique;
    int nsample;
    float eps, momentum;
} pda_densitynet_scale_t;
int pda_densitynet_fwd_multi(const pda_densitynet_scale_t *scales, int nscales, pda_stream_t stream);
int pda_densitynet_bwd_multi(const pda_densitynet_scale_t *scales, int nscales, pda_stream_t stream);

/* Inference: the three layers with their BatchNorms folded in (running statistics), one launch, one thread per token.
 * folded (pda_densitynet_eval_param_count() = 177 floats): w1[16] b1[16] W2[8][16] b2[8] w3[8] b3 with
 * W' = W * gamma / sqrt(running_var + eps), b' = (bias - running_mean) * gamma / sqrt(running_var + eps) + beta. */
int pda_densitynet_eval_param_count(void);
int pda_densitynet_eval(const float *x, const float *folded, float *y, int64_t n, pda_stream_t stream);

/* PDA grouper geometry (MI355X extension; pointnet2_utils.py:590-607, pointnet2_modules.py:905-913,:1000-1001),
 * point-major: xyz (B,N,3), new_xyz (B,M,3), idx (B,M,nsample) -> rppe (B,M,nsample,12) = [centre, neighbour,
 * centre - neighbour, (neighbour - centre) / radius] and dscale (B,M,nsample) = gaussian density
 * exp(-|d|^2 / (2 r^2)) / (2.5 r) divided by its maximum over the group.  nsample: power of two <= 64. */
int pda_pda_geometry(const float *xyz, const float *new_xyz, const int32_t *idx, float *rppe, float *dscale,
                     int b, int n, int m, int nsample, float radius, pda_stream_t stream);

/* ---- target assignment ------------------------------------------------------------------------
 * replaces points_in_boxes_gpu (pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:98-118 ->
 * roiaware_pool3d_kernel.cu:313-359; test :16-36): boxes (B,T,7) [x,y,z,dx,dy,dz,heading],
 * pts (B,M,3) -> box_idx_of_points (B,M) int32 = lowest k whose box contains the point
 * (|z-cz| <= dz/2, |local x| < dx/2 + 1e-5, |local y| < dy/2 + 1e-5 after rotating by -heading);
 * entries of points in no box are NOT written (the caller pre-fills -1, roiaware_pool3d_utils.py:41). */
int pda_points_in_boxes(const float *boxes, const float *pts, int32_t *box_idx_of_points, int b, int t,
                        int m, pda_stream_t stream);
/* ---- RoI pooling of the two-stage heads (csrc/roi_pool.hip) ------------------------------------------
 * roiaware_pool3d (roiaware_pool3d_kernel.cu:39-233): rois (N,7), pts (P,3), pts_feature (P,C) ->
 * pts_idx_of_voxels (N,ox,oy,oz,K) int32 [slot 0: the voxel's count, capped at K-1; slots 1..count: its first K-1
 * points in ascending point index], pooled_features (N,ox,oy,oz,C) and, for pool_method 0 (max), argmax
 * (N,ox,oy,oz,C) int32 (-1 for an empty voxel, whose pooled_features are not written); pool_method 1 (avg) is the
 * float32 sum in slot order divided once by the count and leaves argmax alone.  The caller zero-fills the three
 * outputs.  A point is in a box by the test of pda_points_in_boxes; its voxel follows the reference's float32
 * expressions, unsigned clamp included.  ox, oy, oz in 1..255, K >= 1.  Two runs give the same bits. */
int pda_roiaware_pool3d_fwd(const float *rois, const float *pts, const float *pts_feature, int32_t *argmax,
                            int32_t *pts_idx_of_voxels, float *pooled_features, int boxes_num, int pts_num,
                            int channels, int max_pts_each_voxel, int out_x, int out_y, int out_z, int pool_method,
                            pda_stream_t stream);
/* roiaware_pool3d backward (:236-310): grad_in (P,C), zero-filled by the caller, += grad_out at argmax (max, -1
 * skipped) or grad_out * (1 / max(count, 1)) at every slot's point (avg); float atomics.  Point indices outside
 * [0, pts_num) are skipped. */
int pda_roiaware_pool3d_bwd(const int32_t *pts_idx_of_voxels, const int32_t *argmax, const float *grad_out,
                            float *grad_in, int boxes_num, int pts_num, int channels, int max_pts_each_voxel,
                            int out_x, int out_y, int out_z, int pool_method, pda_stream_t stream);
/* roipoint_pool3d (roipoint_pool3d_kernel.cu:38-165): xyz (B,P,3), boxes3d (B,M,7) already enlarged, pts_feature
 * (B,P,C) -> pooled_features (B,M,S,3+C): the rows [x, y, z, features] of the first S points inside each box in
 * ascending index, slot k >= cnt repeating slot k % cnt; pooled_empty_flag (B,M) int32 = 1 for a box without points,
 * whose rows are not written.  The caller zero-fills both.  S <= 15360, B <= 65535. */
int pda_roipoint_pool3d_fwd(const float *xyz, const float *boxes3d, const float *pts_feature, float *pooled_features,
                            int32_t *pooled_empty_flag, int batch_size, int pts_num, int boxes_num, int channels,
                            int sampled_pts_num, pda_stream_t stream);
/* points_in_boxes_cpu (roiaware_pool3d.cpp:128-168) on the device: boxes (N,7), pts (P,3) -> mask (N,P) int32 of
 * 0 / 1, every entry written; the host statement of the test: margin 1e-2, no FMA. */
int pda_points_in_boxes_mask(const float *boxes, const float *pts, int32_t *mask, int boxes_num, int pts_num,
                             pda_stream_t stream);
/* What SECONDNetIoU's num_pts_iou_cls score does on the CPU (points_in_boxes_cpu(...).sum(1) per scene), for the batch in
 * one launch: points (N, stride) float32 rows [batch, x, y, z, ...] with stride >= 4, boxes (B, M, 7) -> counts (B, M) int32,
 * every entry written, = the points of scene b that the test of pda_points_in_boxes_mask puts inside box (b, m).  A point
 * whose batch value is outside [0, B) or not a number counts nowhere.  Integer sums: the result depends on no order.
 * B <= 65535. */
int pda_points_in_boxes_count(const float *points, int stride, const float *boxes, int32_t *counts, int pts_num,
                              int batch_size, int boxes_num, pda_stream_t stream);
/* The point-wise remainder of the IA-SSD head's target assignment (IASSD_head.py:132-277 after the two points_in_boxes
 * queries), one launch per point set: from in_box / in_ext (B, N) = index of the ground-truth box / enlarged box each point
 * lies in (-1: none) and gt_boxes (B, T, 8) [x y z dx dy dz heading class]:
 *   mode 0 (set_ignore_flag, :207-217)   foreground = in a box; points only inside the enlarged box get label -1
 *   mode 1 (use_ex_gt_assign, :190-205)  foreground = in an enlarged box; instance points keep their own box index
 *   mode 2 (mode 1 + fg_pc_ignore)       foreground = in the enlarged box only; box index -1 for the instance points
 * labels (B*N) int64: 0 background, -1 ignored, else the class of the box (1 when single_class); box_idx (B*N) int64;
 * gt_of_points (B*N, 8) = gt_boxes[scene][box index], index -1 wrapping to the last row as the reference's indexing does. */
int pda_assign_point_targets(const float *gt_boxes, const int32_t *in_box, const int32_t *in_ext, int64_t *labels,
                             int64_t *box_idx, float *gt_of_points, int b, int n, int t, int mode, int single_class,
                             pda_stream_t stream);
/* Soft instance labels of gauss_fun_once_topk_GT_add_same_size (IASSD_head.py:889-963): out[p] = exp(-0.5 |S d|^2) where
 * labels[p] > 0, else 0; d = offset of point p (coords + p*stride + offset: x, y, z) in the frame of its box
 * gt_of_points[p], S = diag(4/(w^2+l^2), 4/(w^2+h^2), 4/(h^2+l^2)) times 4 / 6 / 5 for classes 1 / 2 / 3. */
/* assign_stack_targets_IASSD (IASSD_head.py:132-277) for one point set in one launch: both box queries (boxes, and boxes
 * enlarged by extra_width[3] -- a HOST pointer), labels / box index / gathered box, and (box_labels != NULL) the box-coder
 * targets of the foreground points.  points: rows of point_stride floats, xyz at point_offset (b * n rows, scene-major). */
int pda_head_assign_targets(const float *points, int point_stride, int point_offset, const float *gt_boxes, const float *extra_width,
                            int64_t *labels, int64_t *box_idx, float *gt_of_points, float *box_labels, const float *mean_size,
                            int bins, int b, int n, int t, int mode, int single_class, pda_stream_t stream);
int pda_sa_gaussian_mask(const float *coords, int stride, int offset, const float *gt_of_points, const int64_t *labels,
                         float *out, int64_t points, pda_stream_t stream);

/* ---- rotated BEV overlap / IoU / NMS (pcdet/ops/iou3d_nms) --------------------------------------
 * replace boxes_overlap_bev_gpu / boxes_iou_bev_gpu (src/iou3d_nms.cpp:40-63 / :65-87 ->
 * iou3d_nms_kernel.cu:236-264): boxes_a (num_a,7), boxes_b (num_b,7) [x,y,z,dx,dy,dz,heading] ->
 * (num_a,num_b) BEV intersection area / IoU. */
int pda_boxes_overlap_bev(const float *boxes_a, const float *boxes_b, float *ans_overlap, int num_a,
                          int num_b, pda_stream_t stream);
int pda_boxes_iou_bev(const float *boxes_a, const float *boxes_b, float *ans_iou, int num_a, int num_b,
                      pda_stream_t stream);
/* replaces nms_gpu / nms_normal_gpu (src/iou3d_nms.cpp:90-138 / :141-188 -> kernels :266-369), for a
 * whole batch and without the reference's device->host mask copy: boxes (B,N,7), each scene already
 * sorted by descending score; num_valid (B) int32 or NULL = only the first num_valid[s] boxes of a
 * scene take part; keep (B,N) int64 = kept indices in score order, padded with -1; num_keep (B) int32.
 * normal != 0: axis-aligned IoU (nms_normal_gpu).  mask_scratch: B * pda_nms_mask_words(N) uint64.
 * N <= 32768. */
int64_t pda_nms_mask_words(int n);
int pda_nms_bev(const float *boxes, const int32_t *num_valid, int64_t *keep, int32_t *num_keep,
                uint64_t *mask_scratch, int b, int n, float thresh, int normal, pda_stream_t stream);
/* The result of model_nms_utils.multi_classes_nms for a batch, in one launch behind one pda_nms_bev over b * c problems (scene
 * s, problem p = a class column of a head, head after head): boxes (b * c, k, 7) and scores (b * c, k) sorted as pda_nms_bev
 * saw them, keep (b * c, k) and num_keep (b * c) its outputs, label_map (c) int32 the 1-based label of each problem.  Scene s
 * receives, problem after problem, the first min(num_keep, post_max) kept boxes of each in score order: pred_boxes
 * (b, c * cap, 7), pred_scores (b, c * cap), pred_labels (b, c * cap) int64, cap = min(post_max, k); the rows behind them
 * are zero (label 0 = padding); num_pred (b) int32.  c <= 256. */
int pda_multi_nms_compact(const float *boxes, const float *scores, const int64_t *keep, const int32_t *num_keep,
                          const int32_t *label_map, int b, int c, int k, int post_max, float *pred_boxes, float *pred_scores,
                          int64_t *pred_labels, int32_t *num_pred, pda_stream_t stream);
/* pda_multi_nms_compact for boxes (b * c, k, box_cols) and pred_boxes (b, c * cap, box_cols), box_cols in 7..9 (7 + custom
 * columns): the same launch, every column of a kept row copied.  pda_nms_bev keeps reading 7-column rows, so the caller hands
 * it a contiguous copy of columns 0..6 of the same rows and this entry the full rows; keep indexes both alike. */
int pda_multi_nms_compact_wide(int box_cols, const float *boxes, const float *scores, const int64_t *keep,
                               const int32_t *num_keep, const int32_t *label_map, int b, int c, int k, int post_max,
                               float *pred_boxes, float *pred_scores, int64_t *pred_labels, int32_t *num_pred,
                               pda_stream_t stream);

/* ---- loss terms of the IA-SSD head, one launch each: the term AND its gradient (csrc/head_loss.hip) --------------------------
 * Replace the elementwise torch chains of IASSD_head.py:525-735, :1239-1321 and loss_utils.py:75-194, :340-363.  All tensors
 * row-major f32 unless noted; labels int64; every `grad` output has the layout of the prediction it belongs to and is written
 * completely; the autograd node multiplies it by the incoming scalar.
 *   pda_head_cls_loss:    out2 = {scale * sum_rows w_row * mean_c bce(x, t), #positives}; w_row = [label >= 0] / max(#pos, 1),
 *                         t = [label == c + 1] * soft_row (soft may be NULL = 1); the C logits sit in columns col0 .. col0+C-1
 *                         of rows of row_stride floats.
 *   pda_head_centerness:  generate_center_ness_mask (:795-817); centers (n, 4) [bs, x, y, z], gt (n, 8).
 *   pda_head_box_loss:    get_center_box_binori_layer_loss; preds (n, 6 + 2 bins), labels (n, 8); out4 = {total, xyzwhl,
 *                         ori_bin * dir_weight, ori_res}; code_weights 6 floats or NULL.
 *   pda_head_vote_loss:   mode 0 get_contextual_vote_loss (key = class label of the point), mode 1 _ver2 (key = box index, -1
 *                         none; b scenes of n / b points, `boxes` boxes per scene); origin, offsets, grad (n, 4) [bs, x, y, z].
 *   pda_head_corner_loss: get_corner_layer_loss incl. the decode of PointResidual_BinOri_Coder (mean_size (num_class, 3) or
 *                         NULL); NaN without positive centres, like the reference. */
int pda_head_cls_loss(const float *preds, int row_stride, int col0, int num_class, const int64_t *labels, const float *soft,
                      int64_t n, float scale, float *out2, float *grad, pda_stream_t stream);
int pda_head_centerness(const float *centers, const float *gt, const int64_t *labels, float *out, int64_t n, pda_stream_t stream);
int pda_head_box_loss(const float *preds, const float *labels, const int64_t *cls_labels, const float *code_weights, float beta,
                      int bins, float dir_weight, float box_weight, int64_t n, float *out4, float *grad, pda_stream_t stream);
int pda_head_vote_loss(int mode, const float *origin, const float *offsets, const int64_t *key, const float *gt, int b, int boxes,
                       int num_class, float weight, int64_t n, float *out1, float *grad, pda_stream_t stream);
int pda_head_corner_loss(const float *box_preds, const float *centers, const float *cls_preds, int num_class, const float *gt,
                         const int64_t *cls_labels, const float *mean_size, int bins, float weight, int64_t n, float *out1,
                         float *grad_box, float *grad_centers, pda_stream_t stream);

/* ---- the NARROW vanilla set-abstraction scale in training form (csrc/sa_train_small.hip; MI355X extension) -------------
 * QueryAndGroup -> [Conv2d 1x1 (no bias) -> BatchNorm2d (batch statistics) -> ReLU] x 3 -> max over nsample
 * (pointnet2_modules.py:1657-1670, pointnet2_utils.py:671-704) for chains 3 + c -> c1 -> c2 -> c3 with c <= 5,
 * c1, c2 in {16, 32} and (nsample, c3) in {(16, 32), (32, 64)}: ONCE / KITTI layer 0.  Forward and backward are families
 * of recompute passes over the neighbour lists: no (B, M, ns, C) tensor exists in HBM in the forward pass, the backward
 * pass keeps dz2 (tokens, c2) and dz1 (tokens, c1) only (tokens = b * m * nsample, a multiple of 32).
 *   fwd: out (b*m, c3) = the pooled activation, zmax = the layer-3 pre-activation at the arg-max, arg = the arg-max slot
 *        (lowest slot on ties); running statistics of the three BatchNorms updated (entries of running_* may be NULL);
 *        `workspace` (pda_sa_small_train_workspace_bytes(), 256-byte aligned) receives the packed weights and the batch
 *        statistics and must reach the backward call unchanged.
 *   bwd: grad_out (b*m, c3) -> dw1 (c1, 3 + c), dw2 (c2, c1), dw3 (c3, c2), dgamma[l] / dbeta[l] (l = 0..2).  The
 *        gradient wrt the gathered inputs (xyz, features) is NOT produced: layer 0's inputs are the raw points.
 * feat_pm is point-major (b, n, c); with c == 1 that is the memory of the reference's (b, 1, n).
 * Returns PDA_ERR_UNSUPPORTED for any other shape (pda_sa_small_train_supported tells without a call). */
int64_t pda_sa_small_train_workspace_bytes(void);
int pda_sa_small_train_supported(int c, int nsample, int c1, int c2, int c3, int64_t tokens);
int pda_sa_small_train_fwd(const float *xyz, const float *new_xyz, const float *feat_pm, const int32_t *idx,
                           const float *w1, const float *w2, const float *w3, const float *const *gamma,
                           const float *const *beta, float *const *running_mean, float *const *running_var,
                           const float *eps, const float *momentum, void *workspace, float *out, float *zmax,
                           uint8_t *arg, int b, int n, int m, int c, int nsample, int c1, int c2, int c3,
                           pda_stream_t stream);
int pda_sa_small_train_bwd(const float *xyz, const float *new_xyz, const float *feat_pm, const int32_t *idx,
                           const float *grad_out, const float *zmax, const uint8_t *arg, void *workspace, float *dz2,
                           float *dz1, float *dw1, float *dw2, float *dw3, float *const *dgamma, float *const *dbeta,
                           int b, int n, int m, int c, int nsample, int c1, int c2, int c3, pda_stream_t stream);

/* ---- the coordinate columns of a vanilla SA scale's first layer, backward (csrc/sa_xyz_grad.hip; MI355X extension) ----
 * z1 = [xyz[idx] - new_xyz | features[idx]] W1^T, W1 (c1, ldw >= 3 + C).  From grad_z1 (b*m*nsample, c1):
 * dw[o][0:3] (row stride lddw) = sum over tokens of grad_z1[t][o] * (xyz[idx[t]] - new_xyz[centre(t)]) and, when
 * grad_new_xyz (b, m, 3) is not NULL, grad_new_xyz[centre] = -(sum over the centre's samples of grad_z1) W1[:, 0:3].
 * One pass over grad_z1; the feature columns go through pda_linear_wgrad / pda_gemm_split. */
int64_t pda_sa_xyz_grad_scratch_bytes(int c1);
/* Forward of the same layer without a per-token contraction (a linear layer commutes with the gather):
 * z (b*m*nsample, c1) = point_rows[idx] + W1[:, 0:3] (xyz[idx] - new_xyz[centre]), with point_rows (b*n, c1) = features W1[:, 3:]^T
 * computed once per point by the caller (pda_gemm_split); optional bias (c1) and ReLU (inference: BatchNorm folded into W1).
 * c1 in {128, 256, 512, 1024}. */
int pda_sa_point_gather(const float *point_rows, const float *xyz, const float *new_xyz, const int32_t *idx, const float *w,
                        int ldw, const float *bias, int relu, float *z, int b, int n, int m, int nsample, int c1,
                        pda_stream_t stream);
int pda_sa_xyz_grad(const float *grad_z1, const float *xyz, const float *new_xyz, const int32_t *idx, const float *w, int ldw,
                    float *dw, int lddw, float *grad_new_xyz, void *scratch, int b, int n, int m, int nsample, int c1,
                    pda_stream_t stream);
/* Training: pda_sa_point_gather (no bias, no ReLU; the same z bit for bit) that also emits the BatchNorm statistics of what it
 * stores: partial [pda_sa_point_gather_stats_blocks(b*m*nsample, c1)][2][c1] doubles = per-channel sum and sum of squares per
 * workgroup, fixed summation order; finish with pda_bn_finalize_fwd (count = b*m*nsample). */
int64_t pda_sa_point_gather_stats_blocks(int64_t tokens, int c1);
int pda_sa_point_gather_stats(const float *point_rows, const float *xyz, const float *new_xyz, const int32_t *idx,
                              const float *w, int ldw, float *z, double *partial, int b, int n, int m, int nsample, int c1,
                              pda_stream_t stream);
/* The whole backward of that layer behind a training-mode BatchNorm + ReLU in one pass.  grad_a1 (b*m*nsample, c1): the gradient
 * at relu(bn(z1)); z1, mean_invstd (2, c1), gamma, beta: the layer's forward; bwd_sums (2, c1): pda_bn_relu_bwd_reduce's.  The
 * gradient at z1 is formed per element (pda_bn_relu_bwd's expression) and never written: it yields dw[:, 0:3] and grad_new_xyz
 * (may be NULL) as pda_sa_xyz_grad does, and is scatter-added onto grad_points (b, n, c1) by idx -- the gradient of point_rows,
 * cleared by this call (float atomics: the order of the additions to one point is not fixed).
 * scratch: pda_sa_xyz_grad_scratch_bytes(c1).  c1 <= 1024. */
int pda_sa_point_grad_bn(const float *grad_a1, const float *z1, const float *mean_invstd, const float *gamma,
                         const float *beta, const float *bwd_sums, const float *xyz, const float *new_xyz, const int32_t *idx,
                         const float *w, int ldw, float *dw, int lddw, float *grad_new_xyz, float *grad_points, void *scratch,
                         int b, int n, int m, int nsample, int c1, pda_stream_t stream);

/* ---- the input stage of the data loader (csrc/input_stage.hip; the reference's DataProcessor
 * mask_points_and_boxes_outside_range -> sample_points -> shuffle_points chain and collate_batch, on the device) ----------
 * points (n_total, C >= 3) [x, y, z, features...] holds `batch` scenes back to back; offsets (batch + 1) int64 on the
 * device, scene b = rows [offsets[b], offsets[b+1]), at most n_cap rows each.  range6 (HOST) = [xmin, ymin, zmin, xmax,
 * ymax, zmax].  out_points (batch * num_points, 1 + C) = [b, x, y, z, features...]; per scene: the points with
 * xmin <= x <= xmax and ymin <= y <= ymax (z not tested), near = sqrt((x*x + y*y) + z*z) < 40, and with n masked,
 * n_far far points, k = num_points:
 *   (A) n > k, n_far < k: choice = near[pick[0 .. k-n_far)] ++ far;  (B) n > k, n_far >= k: choice = masked[pick[0 .. k)];
 *   (C) n <= k: choice = masked ++ masked[pick[0 .. k-n)];
 *   out[b][j] = choice[perm1[perm2[j]]]  (perm2 omitted when shuffle == 0).
 * Explicit mode: pick, perm1 (and perm2 exactly when shuffle == 1) are int32 (batch, num_points) on the device; ranks
 *   out of range yield a zero row and status bit 8.  Seeded mode (pick == perm1 == perm2 == NULL): the draws are generated
 *   from `seed` (keyed bijections for the samples without replacement and the shuffles, a counter hash for case C).
 * info (batch, 4) int32 = [n, n_far, kept boxes, status]: this entry writes columns 0, 1, 3; status bits: 1 no point in
 *   range (the reference raises), 2 offsets outside [0, n_total], 4 more than n_cap raw points (2 and 4: the scene is
 *   treated as empty), 8 a draw out of range.  Rows of a scene with a status are [b, 0...].
 * workspace: pda_input_stage_workspace_bytes(batch, n_cap) bytes, 4-byte aligned (-1: bad sizes).  Four launches, no
 * host synchronisation; the grids depend on batch, n_cap and num_points only (graph-capturable). */
int64_t pda_input_stage_workspace_bytes(int batch, int64_t n_cap);
int pda_input_stage(const float *points, const int64_t *offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                    const float *range6, int num_points, const int32_t *pick, const int32_t *perm1, const int32_t *perm2,
                    uint64_t seed, int shuffle, float *out_points, int32_t *info, void *workspace, pda_stream_t stream);
/* Boxes (m_total, box_dim >= 7) [x, y, z, dx, dy, dz, heading, ...], box_offsets (batch + 1) int64 on the device: a box is
 * kept when at least min_num_corners of its 8 corners lie inside all six limits of range6 (inclusive; 0 keeps every box),
 * the kept boxes of scene b are compacted in order into gt_boxes (batch, max_gt, box_dim), zero-padded; info[b][2] = the
 * kept count (may exceed max_gt: the excess is dropped), -1 when the scene's box offsets are unusable.  One launch. */
int pda_input_boxes(const float *boxes, const int64_t *box_offsets, int64_t m_total, int batch, int box_dim, int max_gt,
                    const float *range6, int min_num_corners, float *gt_boxes, int32_t *info, pda_stream_t stream);

/* ---- the training-time augmentor (csrc/augment.hip; the reference's DataAugmentor gt_sampling -> random_world_flip ->
 * random_world_rotation -> random_world_scaling -> limit_period, then prepare_data's class filter, on the device) ------
 * Scenes: points (n_total, C) + offsets (batch + 1) int64 as for pda_input_stage (at most n_cap rows a scene); boxes
 * (m_total, 8) [x, y, z, dx, dy, dz, heading, class] + box_offsets (batch + 1) int64, class 0 = a name outside
 * CLASS_NAMES (counts for collisions, dropped from the output).
 * Database: db_points (db_n_points, C) float32 object points relative to their box centre, db_offsets (n_obj + 1) int64,
 * db_boxes (n_obj, 7) float32, db_centre (n_obj, 3) float64 (box3d_lidar[:3] as stored), db_class (n_obj) int32 >= 1.
 * Plan (device): cand (batch, k) database ids grouped by class group in SAMPLE_GROUPS order, -1 = no candidate;
 * cand_group (batch, k) the group of each slot (ascending along a row); cand_dz (batch, k) float64 the road-plane shift
 * mv_height (0 without road plane); flip (batch, 2) int32 [flip_x, flip_y]; angle (batch) float64 (0: no rotation);
 * scale (batch) float32 (1: no scaling).  remove_extra_width (HOST) float[3].  k <= 256.
 * A candidate is accepted iff its BEV IoU is 0 with every existing box, with every other candidate of its group and with
 * every accepted candidate of an earlier group.  Scene points inside an accepted box enlarged by remove_extra_width
 * (the CPU test points_in_boxes_cpu: margin 1e-2) are removed.  Output scene b = out_points rows
 * [out_offsets[b], out_offsets[b+1]): the accepted objects' points (the centre added in double, then - dz), in
 * acceptance order, then the kept scene points in their order; out_boxes (.., 8) rows [out_box_offsets[b], ..[b+1]):
 * the existing boxes of class >= 1 in order, then the accepted ones.  Both go through flip_x (y = -y, h = -h), flip_y
 * (x = -x, h = -(h + pi)), the rotation ([x, y] times [[c, s], [-s, c]], h += angle), the scaling (xyz and box dims
 * times scale) and, for the heading, limit_period(h, 0.5, 2 pi), each a separately rounded float32 operation.
 * paste_cap >= the largest total of object points of one scene's candidates (the write grid); out_cap / out_box_cap =
 * the rows of out_points / out_boxes (n_total + batch * paste_cap / m_total + the candidates always suffice).
 * info (batch, 4) int32 = [points out, boxes out, accepted candidates, status]; status bits: 1 no box left (the reference
 * draws another scene), 2 offsets outside the packed points or boxes, 4 more than n_cap points or an output capacity
 * exceeded, 8 a candidate id outside the database or candidate groups out of order (the candidate is ignored).  A scene
 * with bit 2 or 4 is written empty.
 * workspace: pda_augment_workspace_bytes(batch, n_cap, k) bytes, 256-byte aligned (-1: bad sizes).  Four launches, no
 * host synchronisation. */
int64_t pda_augment_workspace_bytes(int batch, int64_t n_cap, int k);
int pda_augment(const float *points, const int64_t *offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                const float *boxes, const int64_t *box_offsets, int64_t m_total, const float *db_points,
                const int64_t *db_offsets, int64_t db_n_points, const float *db_boxes, const double *db_centre,
                const int32_t *db_class, int n_obj, const int32_t *cand, const int32_t *cand_group, const double *cand_dz,
                int k, const int32_t *flip, const double *angle, const float *scale, const float *remove_extra_width,
                int64_t paste_cap, float *out_points, int64_t out_cap, int64_t *out_offsets, float *out_boxes,
                int64_t out_box_cap, int64_t *out_box_offsets, int32_t *info, void *workspace, pda_stream_t stream);

/* The paste-only form of pda_augment, in front of pda_augment_steps: the same collision test, point removal and paste,
 * but no transform, no limit_period, and boxes of class 0 stay in the output (they take part in the steps that follow).
 * Arguments, workspace and info as for pda_augment, without flip / angle / scale. */
int pda_augment_paste(const float *points, const int64_t *offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                      const float *boxes, const int64_t *box_offsets, int64_t m_total, const float *db_points,
                      const int64_t *db_offsets, int64_t db_n_points, const float *db_boxes, const double *db_centre,
                      const int32_t *db_class, int n_obj, const int32_t *cand, const int32_t *cand_group,
                      const double *cand_dz, int k, const float *remove_extra_width, int64_t paste_cap, float *out_points,
                      int64_t out_cap, int64_t *out_offsets, float *out_boxes, int64_t out_box_cap,
                      int64_t *out_box_offsets, int32_t *info, void *workspace, pda_stream_t stream);

/* ---- the augmentor's ordered step program (csrc/augment_steps.hip; the reference's random_world_flip / _rotation /
 * _scaling / _translation / _frustum_dropout and random_local_translation / _rotation / _scaling / _frustum_dropout of
 * pcdet/datasets/augmentor/augmentor_utils.py, in any order, then limit_period and prepare_data's class filter) --------
 * Scenes and boxes as for pda_augment (boxes (m_total, 8), class 0 takes part in every step and is dropped at the end).
 * ops (HOST) (n_ops, 2) int32 [code, arg], n_ops <= 32, run in order:
 *   0 flip_x, 1 flip_y, 2 world rotation, 3 world scaling, 4 world translation (arg: axis 0..2), 5 world frustum dropout
 *   (arg: 0 top, 1 bottom, 2 left, 3 right; at most 4 such ops), 6 local translation (arg: axis), 7 local rotation,
 *   8 local scaling, 9 local frustum dropout (arg: direction).
 *   10 hold (arg 0), as the LAST op only: it is one of the n_ops <= 32 ops, but no step and no column of scene_draws
 *   (which is (batch, n_ops - 1) then); the boxes leave with their headings as they are and class 0 kept, for pda_pyramid_aug behind it.
 * scene_draws (batch, n_ops) float64 on the device: the scene's draw of op i (flip 0 / 1, angle with 0 = off, scale with
 *   1 = off, translation offset, dropout intensity; unused for local ops).  box_draws (batch, n_local, draw_cap) float64:
 *   row l belongs to the l-th local op (codes 6..9) of the program; draw j of a row belongs to the j-th box alive at
 *   that op, in order (a world dropout removes boxes).
 * A local op walks the scene's boxes in order, each box tested against the points as they are then (get_points_in_box:
 * margin 1e-1 on x and y, <= on all axes); box_slots (<= 256) bounds the boxes of one scene: a scene with more boxes, or
 * with more alive boxes than draw_cap at a local op, gets status bit 4 and is written empty.
 * info_in (batch, 4) int32 or NULL: the info of the pda_augment_paste call that made the input; column 2 and the status
 * bits 2, 4, 8 are carried into info.  Output, out_cap / out_box_cap and info as for pda_augment (points never grow:
 * n_total / m_total rows suffice); status bit 1: no box or no point left.
 * workspace: pda_augment_steps_workspace_bytes(batch, n_cap, box_slots, n_ops) bytes, 256-byte aligned (-1: bad sizes).
 * 2 * (world dropout ops) + 4 launches, no allocation, no host synchronisation. */
int64_t pda_augment_steps_workspace_bytes(int batch, int64_t n_cap, int box_slots, int n_ops);
int pda_augment_steps(const float *points, const int64_t *offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                      const float *boxes, const int64_t *box_offsets, int64_t m_total, const int32_t *ops, int n_ops,
                      const double *scene_draws, const double *box_draws, int draw_cap, int box_slots,
                      const int32_t *info_in, float *out_points, int64_t out_cap, int64_t *out_offsets, float *out_boxes,
                      int64_t out_box_cap, int64_t *out_box_offsets, int32_t *info, void *workspace, pda_stream_t stream);

/* ---- random_local_pyramid_aug (csrc/augment_steps.hip; the reference's local_pyramid_dropout -> local_pyramid_sparsify ->
 * local_pyramid_swap of augmentor_utils.py, then limit_period and prepare_data's class filter) ---------------------------
 * Scenes and boxes as pda_augment_steps leaves them behind a hold op: boxes (m_total, 8), class 0 takes part and is
 * dropped at the end; boxes are never changed.  C >= 4: the swap rescales the LAST column.  A box is six pyramids (apex the
 * centre, base a face: 0 +x, 1 +z, 2 -x, 3 -z, 4 -y, 5 +y in the box frame); a point is in the pyramid of the largest of
 * |lx / (dx / 2)|, |ly / (dy / 2)|, |sz / (dz / 2)| when all are <= 1 (get_points_in_box's rotation, no margin).
 * Draws (device), draw_cap <= 256 columns a row, n_draws (batch, 3) int32 the draws present in the dropout / sparsify /
 * swap rows of a scene:
 *   draws_f64 (batch, 5, draw_cap): dropout u, sparsify u, swap u, swap face u, swap partner u (the last two in [0, 1)).
 *   draws_i32 (batch, 4, draw_cap): dropout face, sparsify face (0..5), explicit swap face or -1, explicit swap partner
 *     (an index among the boxes in front of the swap) or -1.
 *   sparsify_key (batch, draw_cap) uint64; sparsify_keep (batch, draw_cap, 1 + sparsify_max) int32 or NULL: [length,
 *     ranks...], length 0 = use the key.
 * Draw j of the dropout row belongs to box j; of the sparsify row to the j-th box not dropped; of the swap rows to the j-th
 * box neither dropped nor selected by the sparsify.  probs (HOST) double[3] = DROP_PROB, SPARSIFY_PROB, SWAP_PROB (u <= p
 * selects).  A dropped box loses the points of its drawn pyramid.  A sparsify-selected pyramid with more than
 * sparsify_max points (counted after the dropout, ranked in scene order) keeps the ranks of its keep list, or rank r iff
 * keyed_bijection(key, count, r) < sparsify_max; a point is thinned away iff it lies in a thinned pyramid and none that
 * holds it keeps it.  A swap-selected box takes face floor(u * k) of its k faces with count > swap_max (counts and
 * min / max of the last column on the survivors), then partner floor(u * k) of the k boxes left whose same face has
 * count > swap_max and is no to-swap pyramid, or itself without one; the points of both pyramids change places by their
 * ratios in the pyramid frames, the last column rescaled to the other pyramid's range.  Pairs act in ascending box order:
 * a self pair and a pair whose partner pyramid an earlier pair holds do nothing, a point in pyramids of several pairs is
 * moved by the first.  A scene never grows.
 * Status bit 16: a row with fewer draws than boxes, a face outside 0..5, a keep list of the wrong length or with a
 * repeated or out-of-range rank, an explicit face without count > swap_max, an explicit partner that is no candidate
 * (without candidates: not the box itself); the scene is written empty.  Output, info, info_in, capacities and the other
 * status bits as for pda_augment_steps; points come out in scene order.
 * workspace: pda_pyramid_aug_workspace_bytes(batch, n_cap, box_slots) bytes, 256-byte aligned (-1: bad sizes).  Seven
 * launches, no allocation, no host synchronisation. */
int64_t pda_pyramid_aug_workspace_bytes(int batch, int64_t n_cap, int box_slots);
int pda_pyramid_aug(const float *points, const int64_t *offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                    const float *boxes, const int64_t *box_offsets, int64_t m_total, const double *draws_f64,
                    const int32_t *draws_i32, const uint64_t *sparsify_key, const int32_t *sparsify_keep,
                    const int32_t *n_draws, int draw_cap, const double *probs, int sparsify_max, int swap_max,
                    int box_slots, const int32_t *info_in, float *out_points, int64_t out_cap, int64_t *out_offsets,
                    float *out_boxes, int64_t out_box_cap, int64_t *out_box_offsets, int32_t *info, void *workspace,
                    pda_stream_t stream);

/* ---- ONCE evaluation (csrc/once_eval.hip; the reference's once_eval get_evaluation_results on the device) ------------
 * Frames: GT boxes (n_gt_total, 7) float64 [x, y, z, dx, dy, dz, heading] with gt_name (n_gt_total) int32 name ids and
 * gt_offsets (n_frames + 1) int64; predictions of frame f are rows [pred_start[f], pred_start[f] + pred_count[f]) of
 * pred_boxes (pred_cap, 7) float32, pred_score (pred_cap) float32 and pred_name (pred_cap) int32 (packed or padded
 * storage alike).  The IoU block of frame f is n_gt x pred_count row-major at iou[iou_start[f]], iou_start[f] plus
 * n_gt * pred_count at most iou_cap.  All arrays are on the device; max_gt / max_pred bound every frame (max_pred <= 4096).
 * A frame outside these bounds sets status bit 1 and counts as empty.  A name id outside [0, n_names) sets bit 2 and is
 * rejected by every class. */
typedef struct pda_once_frames {
    const double *gt_boxes;
    const int32_t *gt_name;
    const int64_t *gt_offsets;
    const float *pred_boxes, *pred_score;
    const int32_t *pred_name;
    const int64_t *pred_start;
    const int32_t *pred_count;
    const int64_t *iou_start;
    int64_t n_gt_total, pred_cap, iou_cap;
    int n_frames, max_gt, max_pred;
} pda_once_frames_t;

/* workspace of pda_once_eval_accumulate / pda_once_eval_match for n_tasks = classes x difficulties, 256-byte aligned:
 * the TP-score segments (n_tasks, n_gt_total) float32 at offset 0, then n_tasks int64 TP counts (-1: bad sizes). */
int64_t pda_once_eval_workspace_bytes(int n_frames, int64_t n_gt_total, int n_tasks);
/* 3D IoU of every (GT, prediction) pair of a frame, as the reference's iou3d_kernel(_with_heading): the rotated BEV
 * intersection in float32 (iou_utils.devRotateIoUEval(pred, gt, 2)), the rest in float64; with_heading zeroes pairs whose
 * heading difference folded to [0, pi] exceeds pi / 2.  One launch. */
int pda_once_eval_iou(const pda_once_frames_t *frames, int with_heading, double *iou, int32_t *status,
                      pda_stream_t stream);
/* accumulate_scores for every (frame, class, difficulty): accept (HOST) n_classes x n_names bytes (1: the class takes
 * the name), iou_thr (HOST) n_classes, difficulty_mode 0 'Overall&Distance' (4 levels), 1 'Overall' (1), 2 'Distance'
 * (3); n_classes <= 16, n_names <= 64.  Writes the TP scores of task t = class * n_difficulties + level to workspace
 * segment t at the frame's GT rows, -inf in the rest, the TP counts, and num_valid_gt (n_tasks) int64.  The caller sorts
 * each segment in descending order before pda_once_eval_match. */
int pda_once_eval_accumulate(const pda_once_frames_t *frames, const double *iou, const uint8_t *accept, int n_classes,
                             int n_names, const double *iou_thr, int difficulty_mode, int64_t *num_valid_gt,
                             int32_t *status, void *workspace, pda_stream_t stream);
/* get_thresholds and compute_statistics: sorted_scores (n_tasks, n_gt_total) float32, each row in descending order (the
 * workspace segments sorted); thresholds (n_tasks, num_pr_points + 1) float64, n_thresholds (n_tasks) int64 (more than
 * num_pr_points + 1 sets status bit 4), counts (n_tasks, num_pr_points + 1, 3) int64 tp / fp / fn summed over frames.
 * Same frames, table and mode as pda_once_eval_accumulate.  Two launches. */
int pda_once_eval_match(const pda_once_frames_t *frames, const double *iou, const uint8_t *accept, int n_classes,
                        int n_names, const double *iou_thr, int difficulty_mode, int num_pr_points,
                        const float *sorted_scores, const int64_t *num_valid_gt, double *thresholds,
                        int64_t *n_thresholds, int64_t *counts, int32_t *status, void *workspace, pda_stream_t stream);


/* ---- KITTI evaluation (csrc/kitti_eval.hip; the reference's kitti_object_eval_python get_official_eval_result) -------
 * Frames, in the dtypes of KITTI infos and of generate_prediction_dicts: GT rows gt_bbox (n_gt_total, 4) float32 image
 * box, gt_loc (n_gt_total, 3) float32 camera location, gt_dims (n_gt_total, 3) float64 (l, h, w), gt_ry, gt_alpha,
 * gt_trunc, gt_occ (n_gt_total) float64, gt_name int32 name ids (DontCare rows included), gt_offsets (n_frames + 1)
 * int64.  Detections of frame f are rows [dt_start[f], dt_start[f] + dt_count[f]) of dt_bbox (det_cap, 4), dt_box
 * (det_cap, 7) camera (x, y, z, l, h, w, ry), dt_alpha, dt_score (det_cap) float32 and dt_name (det_cap) int32 (packed
 * or padded storage alike).  The overlap block of frame f is n_gt x dt_count row-major (GT rows, detection columns) at
 * element ov_start[f] of each metric plane; ov_start[f] + n_gt * dt_count at most ov_cap.  frame_mode (n_frames) int32,
 * may be null: bit 1 detection bboxes of the frame's part are float64, 2 GT bboxes float64, 4 detection location /
 * dimensions / rotation_y float64, 8 detection bbox / alpha / score float64 (the part of get_split_parts(n_frames, 100)
 * decides the dtype numpy computes in).  All arrays are on the device; max_det <= 4096.  A frame outside these bounds
 * sets status bit 1 and counts as empty; a name id outside [0, n_names) sets bit 2 and matches no class. */
typedef struct pda_kitti_frames {
    const float *gt_bbox, *gt_loc;
    const double *gt_dims, *gt_ry, *gt_alpha, *gt_trunc, *gt_occ;
    const int32_t *gt_name;
    const int64_t *gt_offsets;
    const float *dt_bbox, *dt_box, *dt_alpha, *dt_score;
    const int32_t *dt_name;
    const int64_t *dt_start;
    const int32_t *dt_count;
    const int64_t *ov_start;
    const int32_t *frame_mode;
    int64_t n_gt_total, det_cap, ov_cap;
    int n_frames, max_gt, max_det;
} pda_kitti_frames_t;

/* Tasks: t = ((metric * n_classes + class) * 3 + difficulty) * 2 + overlap setting, n_tasks = 18 n_classes, metric 0
 * image, 1 BEV, 2 3D; (class, difficulty) cd = class * 3 + difficulty.  Class tables (HOST), n_classes <= 6 and
 * n_names <= 64: gt_class (n_classes, n_names) int8 1 the class, 0 ignored (Van for Car, Person_sitting for Pedestrian),
 * -1 other; dt_class (n_classes, n_names) uint8 1 a detection of the class; dontcare (n_names) uint8; min_overlaps
 * (2, 3, n_classes) float64 [setting][metric][class].
 * workspace: pda_kitti_eval_workspace_bytes(n_frames, n_gt_total, det_cap, n_classes) bytes, 256-byte aligned: the
 * TP-score segments (n_tasks, n_gt_total) float32 at offset 0, then scratch (-1: bad sizes). */
int64_t pda_kitti_eval_workspace_bytes(int n_frames, int64_t n_gt_total, int64_t det_cap, int n_classes);
/* The three overlap planes (3, ov_cap) float64 of every frame's (GT, detection) block: image_box_overlap (criterion -1,
 * in the detection bbox dtype), the BEV rotate_iou of (x, z, l, w, ry) rounded to float32, and d3_box_overlap, the BEV
 * intersection times the height overlap along camera -y, rounded to float32.  One launch. */
int pda_kitti_eval_overlaps(const pda_kitti_frames_t *frames, double *overlaps, int32_t *status, pda_stream_t stream);
/* clean_data and compute_statistics_jit(compute_fp=False): gt_flags (3 n_classes, n_gt_total) and dt_flags
 * (3 n_classes, det_cap) int8 ignored_gt / ignored_det per cd, num_valid_gt (3 n_classes) int64; the TP scores of task t
 * into workspace segment t at the frame's GT rows, -inf in the rest.  The caller sorts each segment in descending order
 * before pda_kitti_eval_match.  Two launches. */
int pda_kitti_eval_first_pass(const pda_kitti_frames_t *frames, const double *overlaps, int n_classes, int n_names,
                              const int8_t *gt_class, const uint8_t *dt_class, const uint8_t *dontcare,
                              const double *min_overlaps, int8_t *gt_flags, int8_t *dt_flags, int64_t *num_valid_gt,
                              int32_t *status, void *workspace, pda_stream_t stream);
/* get_thresholds (41 sample points) and compute_statistics_jit(compute_fp=True): sorted_scores (n_tasks, n_gt_total)
 * float32 rows in descending order; thresholds (n_tasks, 41) float64, n_thresholds (n_tasks) int64 (more than 41 sets
 * status bit 4), counts (n_tasks, 41, 3) int64 tp / fp / fn summed over frames with DontCare suppression on metric 0,
 * similarity (6 n_classes, 41) float64 the AOS sums of the metric-0 tasks in frame order (zero unless compute_aos).  Same
 * frames and tables as pda_kitti_eval_first_pass.  Up to three launches. */
int pda_kitti_eval_match(const pda_kitti_frames_t *frames, const double *overlaps, int n_classes, int n_names,
                         const int8_t *gt_class, const uint8_t *dt_class, const uint8_t *dontcare,
                         const double *min_overlaps, int compute_aos, const int8_t *gt_flags, const int8_t *dt_flags,
                         const float *sorted_scores, const int64_t *num_valid_gt, double *thresholds,
                         int64_t *n_thresholds, int64_t *counts, double *similarity, int32_t *status, void *workspace,
                         pda_stream_t stream);
/* generate_prediction_dicts' geometry, float32: boxes (n, stride) lidar (x, y, z, dx, dy, dz, heading) of frame
 * frame_idx[r], or r / rows_per_frame when frame_idx is null; calib (n_frames, 33) P2 (3 x 4), R0 (3 x 3), V2C (3 x 4)
 * row-major; image_shape (n_frames, 2) int32 (H, W).  Writes cam (n, 7) camera (x, y, z, l, h, w, ry), bbox (n, 4) the
 * projected corners' box clipped to the image, alpha (n).  A frame index outside [0, n_frames) sets status bit 1 and
 * leaves the row unwritten.  One launch. */
int pda_kitti_eval_predictions(const float *boxes, int64_t n, int stride, int rows_per_frame, const int32_t *frame_idx,
                               const float *calib, const int32_t *image_shape, int n_frames, float *cam, float *bbox,
                               float *alpha, int32_t *status, pda_stream_t stream);

/* ---- 3-D recall of the eval loop (csrc/recall.hip) -------------------------------------------------------------------------
 * generate_recall_record (detector3d_template.py:288-329) for b scenes: pred_boxes (b, k, 7) the final boxes after NMS, of
 * which the first num_pred[s] (b int32, clamped to [0, k]) count; gt_boxes (b, t, gt_cols) float32, gt_cols >= 7, each
 * scene trimmed as the reference does (rows 0..j, j the last row in 1..t-1 whose float32 sum != 0, else 0).  A kept GT
 * row's IoU is boxes_iou3d_gpu(pred, gt)'s (iou3d_nms_utils.py:48-84, float32, box_overlap(pred, gt)); it is recalled at
 * threshold i when its max over the predictions > thresh[i].  thresh: HOST float32, 0 <= n_thresh <= 16.  counters
 * (1 + n_thresh) int64 [gt, rcnn_0, ...]: the kernel ADDS the kept rows and the recalled rows, so one buffer can sum an
 * epoch.  max_iou (b, t) or NULL: each kept row's max over the predictions, 0 without predictions; trimmed rows are not
 * written.  One launch, no host read; integer atomics, so runs are bit-identical. */
int pda_recall_record(const float *pred_boxes, const int32_t *num_pred, const float *gt_boxes, int gt_cols,
                      const float *thresh, int n_thresh, int64_t *counters, float *max_iou, int b, int k, int t,
                      pda_stream_t stream);

/* ---- RoI targets of a two-stage head (csrc/roi_targets.hip) ------------------------------------------------------------------
 * ProposalTargetLayer (roi_heads/target_assigner/proposal_target_layer.py) and the canonical transformation of
 * RoIHeadTemplate.assign_targets (roi_head_template.py:104-134) for b scenes, two launches, no host read.  rois (b, m, 7)
 * float32, roi_labels (b, m) int64, gt_boxes (b, t, gt_cols) float32 with gt_cols >= 8: the box in columns 0..6 and the
 * class label in the LAST column; each scene's GT trimmed as for pda_recall_record.  m <= 4096.  Sizes are checked before
 * any pointer is used; b == 0 or m == 0 is PDA_OK and touches nothing.
 *
 * pda_roi_max_iou: max_overlaps (b, m) float32 and gt_assignment (b, m) int32 = max and arg-max of
 * boxes_iou3d_gpu(rois, kept GT) over the kept rows (by_class == 0), or over the kept rows whose int64(label) equals the
 * RoI's label (by_class != 0; 0 / 0 without such a row).  Among equal maxima the lowest row.  t == 0 counts as the
 * reference's single zero box: 0 / 0. */
int pda_roi_max_iou(const float *rois, const int64_t *roi_labels, const float *gt_boxes, int gt_cols, int by_class,
                    float *max_overlaps, int32_t *gt_assignment, int b, int m, int t, pda_stream_t stream);
/* subsample_rois / sample_bg_inds on max_overlaps, then for the roi_per_image picks of each scene (fg, hard bg, easy bg in
 * that order): out_rois (b, r, 7), gt_of_rois_src (b, r, 8) the assigned GT row (columns 0..6 and the label),
 * gt_iou_of_rois (b, r), out_roi_scores (b, r), out_roi_labels (b, r) int64 copied bit for bit; reg_valid_mask (b, r) int64
 * = iou > reg_fg_thresh; rcnn_cls_labels (b, r) int64 for score_type 0 ('cls') or float32 for score_type 1 ('roi_iou');
 * gt_of_rois (b, r, 8) the GT in the RoI's canonical frame with the heading folded into [-pi/2, pi/2]; sampled_inds (b, r)
 * int32 or NULL, the picked RoI of every output row.  Thresholds are rounded to float32 here (torch compares a float32
 * tensor in float32); fg_per_image = int(np.round(FG_RATIO * ROI_PER_IMAGE)) from the caller.  Draws: either all four of
 * perm (b, m) int32 (np.random.permutation(fg_num), first fg_num valid), fg_rand (b, r) float64 (np.random.rand),
 * hard_draw / easy_draw (b, r) int64 (torch.randint, in range) -- the reference's draws, index-exact -- or all four NULL
 * and the draws come from seed.  status (b) int32: 0, 1 for a scene with neither foreground nor background (the reference
 * raises; its rows are zero), 2 for a draw or an assignment out of range (replaced by 0, never followed).  One launch. */
int pda_roi_sample_targets(const float *rois, const float *roi_scores, const int64_t *roi_labels, const float *gt_boxes,
                           int gt_cols, const float *max_overlaps, const int32_t *gt_assignment, int roi_per_image,
                           int fg_per_image, double hard_bg_ratio, double reg_fg_thresh, double cls_fg_thresh,
                           double cls_bg_thresh, double cls_bg_thresh_lo, int score_type, const int32_t *perm,
                           const double *fg_rand, const int64_t *hard_draw, const int64_t *easy_draw, uint64_t seed,
                           float *out_rois, float *gt_of_rois_src, float *gt_of_rois, float *gt_iou_of_rois,
                           float *out_roi_scores, int64_t *out_roi_labels, int64_t *reg_valid_mask, void *rcnn_cls_labels,
                           int32_t *sampled_inds, int32_t *status, int b, int m, int t, pda_stream_t stream);

/* ---- preparing frames (csrc/frame_stage.hip) ---------------------------------------------------------------------------------
 * KittiDataset's FOV_POINTS_ONLY step (kitti_dataset.py get_fov_flag behind calib.lidar_to_rect / calib.rect_to_img) for
 * `batch` scenes in the layout of pda_input_stage: points (n_total, C >= 3), offsets (batch + 1) int64, at most n_cap rows a
 * scene.  calib (batch, 24) float32 on the device: M = V2C^T R0^T (4, 3) row-major, formed by the caller in float32 as
 * Calibration.lidar_to_rect forms it, then P2 (3, 4) row-major.  image_shape (batch, 2) int32 (H, W) on the device.  Per
 * point, in float32 without FMA:
 *   rect_k = ((x*M[0][k] + y*M[1][k]) + z*M[2][k]) + M[3][k];  h_j = ((rx*P2[j][0] + ry*P2[j][1]) + rz*P2[j][2]) + P2[j][3];
 *   u = h_0 / rz, v = h_1 / rz, depth = h_2 - P2[2][3];  kept iff u >= 0 && u < W && v >= 0 && v < H && depth >= 0
 * (a NaN keeps nothing).  out_points (out_cap, C): the kept rows of every scene in their order, bit-identical, back to back
 * (out_cap = n_total always suffices for scenes that do not overlap); out_offsets (batch + 1) int64.
 * info (batch, 4) int32 = [n_in, n_kept, 0, status]; status bits: 2 offsets outside [0, n_total], 4 more than n_cap rows
 * (both: the scene is written empty), 4 also when out_cap is exceeded (rows beyond it are dropped).
 * workspace: pda_kitti_fov_filter_workspace_bytes(batch, n_cap) bytes, 4-byte aligned (-1: bad sizes).  Four launches, no
 * host synchronisation; the grids depend on batch and n_cap only (graph-capturable). */
int64_t pda_kitti_fov_filter_workspace_bytes(int batch, int64_t n_cap);
int pda_kitti_fov_filter(const float *points, const int64_t *offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                         const float *calib, const int32_t *image_shape, float *out_points, int64_t out_cap,
                         int64_t *out_offsets, int32_t *info, void *workspace, pda_stream_t stream);
/* The body of create_groundtruth_database (kitti_dataset.py / once_dataset.py) for `batch` frames: the same points and
 * offsets; boxes (m_total, 7) float32 [x, y, z, dx, dy, dz, heading] with box_offsets (batch + 1) int64, at most 256 boxes a
 * frame; centre (m_total, 3) float64 = gt_boxes[i, :3] as the infos hold it.  Object g (a row of boxes) holds the points of
 * its own frame that pass the CPU test points_in_boxes_cpu (margin 1e-2, no FMA), in point order, each row
 * [(float)((double)x - cx), (float)((double)y - cy), (float)((double)z - cz), features...].  A point may land in several
 * boxes.
 *   pda_gt_extract_count: counts (m_total) int32, 0 for the boxes of a frame with a status;
 *   pda_gt_extract_write: obj_offsets (m_total + 1) int64 = the exclusive scan of counts (made by the caller), obj_points
 *                         (out_cap, C); same arguments and the workspace as pda_gt_extract_count left it.
 * info (batch, 4) int32 = [points, boxes, 0, status]; status bits: 2 point or box offsets outside their buffers, 4 more
 * than n_cap points, 8 more than 256 boxes (all three: the frame is written empty); the write sets 4 when obj_offsets or
 * out_cap do not hold what was counted (such rows are dropped).
 * workspace: pda_gt_extract_workspace_bytes(batch, n_cap, m_total) bytes, 4-byte aligned (-1: bad sizes).  Two launches
 * and one; nothing decides an order but ballots and scans. */
int64_t pda_gt_extract_workspace_bytes(int batch, int64_t n_cap, int64_t m_total);
int pda_gt_extract_count(const float *points, const int64_t *offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                         const float *boxes, const int64_t *box_offsets, int64_t m_total, int32_t *counts, int32_t *info,
                         void *workspace, pda_stream_t stream);
int pda_gt_extract_write(const float *points, const int64_t *offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                         const float *boxes, const int64_t *box_offsets, int64_t m_total, const double *centre,
                         const int64_t *obj_offsets, float *obj_points, int64_t out_cap, int32_t *info, void *workspace,
                         pda_stream_t stream);

/* ---- voxel down-sampling (csrc/voxel_stage.hip; the reference's VoxelGeneratorWrapper.generate -- spconv's CPU
 * point-to-voxel loop -- and DataProcessor.sample_points_by_voxels up to its sample_points call) --------------------------------
 * Scenes in the layout of pda_input_stage: points (n_total, C >= 3), offsets (batch + 1) int64, at most n_cap rows a scene.
 * HOST arrays: range6 = [xmin, ymin, zmin, xmax, ymax, zmax], voxel_size3 = [vx, vy, vz], grid3 = the cells along x, y, z
 * (int32; the caller rounds (range[3:6] - range[0:3]) / voxel_size as the reference does).  Each axis holds 1 .. 2^24 cells
 * and the grid at most 2^32 - 1 cells (the cell key is 32 bits); a larger grid is refused before any launch.
 * Per scene, over the points in order: c_j = floor((p_j - lo_j) / vs_j) in float32 with a correctly rounded division; a
 * point with a c_j outside [0, grid_j) (or NaN) joins nothing; a cell met for the first time becomes the next voxel unless
 * max_voxels voxels exist already (the point is skipped; later points of existing voxels still join); a voxel keeps its
 * first max_points points (1 .. 64).  Voxels are numbered in order of first appearance.
 * workspace: pda_voxel_workspace_bytes(batch, n_cap, max_voxels, max_points) bytes, 8-byte aligned (-1: bad sizes); it holds
 * a hash table of 2^ceil(log2(2 n_cap)) 64-bit entries a scene.  No host synchronisation, no float atomics: the grids depend on
 * batch, n_cap and max_voxels only (graph-capturable) and two runs give the same bits.
 *
 * pda_voxelize: voxels (batch, max_voxels, max_points, C) zero-padded, coords (batch, max_voxels, 3) int32 (z, y, x),
 * num_points_per_voxel (batch, max_voxels) int32, num_voxels (batch) int32 (-1: the scene's offsets are unusable or it holds
 * more than n_cap rows). */
int64_t pda_voxel_workspace_bytes(int batch, int64_t n_cap, int max_voxels, int max_points);
int pda_voxelize(const float *points, const int64_t *offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                 const float *range6, const float *voxel_size3, const int32_t *grid3, int max_voxels, int max_points,
                 float *voxels, int32_t *coords, int32_t *num_points_per_voxel, int32_t *num_voxels, void *workspace,
                 pda_stream_t stream);
/* pda_voxel_sample: [mask_xy: keep xmin <= x <= xmax and ymin <= y <= ymax, z not tested] -> [shuffle: shuffled[s] =
 * masked[perm0[s]]] -> voxelize -> one row a voxel, in voxel order: its first point bit for bit (mean_vfe == 0), or
 * (float)((double)sum / (double)count) per column with sum = the float32 sum over the voxel's max_points slots in slot order
 * (mean_vfe == 1; numpy's voxels.sum(axis=1) / num_points).
 * The shuffle (shuffle == 1): explicit mode takes perm0, ragged int32 with perm0_offsets (batch + 1) int64 into its
 * perm0_total entries, scene b's slice a permutation of [0, n_masked_b); seeded mode (perm0 == perm0_offsets == NULL) draws
 * a keyed bijection of [0, n_masked_b) from `seed`.
 * out_points (out_cap >= batch * min(n_cap, max_voxels), C): the scenes' rows back to back; out_offsets (batch + 1) int64.
 * info (batch, 4) int32 = [n_masked, n_in_grid, n_voxels_before_cap, status]; status bits: 1 no voxel, 2 offsets outside
 * [0, n_total], 4 more than n_cap rows, 8 a bad draw (the perm0 slice has another length than n_masked or an entry outside
 * [0, n_masked)) -- 2, 4, 8: the scene is written empty --, 16 more than max_voxels cells were occupied (not an error: the
 * reference caps silently). */
int pda_voxel_sample(const float *points, const int64_t *offsets, int64_t n_total, int batch, int c, int64_t n_cap,
                     const float *range6, const float *voxel_size3, const int32_t *grid3, int mask_xy, int max_voxels,
                     int max_points, int mean_vfe, int shuffle, const int32_t *perm0, const int64_t *perm0_offsets,
                     int64_t perm0_total, uint64_t seed, float *out_points, int64_t out_cap, int64_t *out_offsets,
                     int32_t *info, void *workspace, pda_stream_t stream);

/* ---- dynamic voxelization (csrc/dyn_voxel.hip; the reference's DynamicMeanVFE / DynamicPillarVFE up to their Linear layers:
 * torch.unique(merge_coords, return_inverse, return_counts) followed by torch_scatter.scatter_mean / scatter_max) -------------
 * points (n, columns >= 4) float32 = the collated [batch_idx, x, y, z, ...] rows, scenes in any order.  HOST arrays range6,
 * voxel_size3, grid3 as pda_voxelize takes them; each axis holds 1 .. 2^24 cells.  pillars == 0: cells in x, y, z;
 * pillars == 1: cells in x and y, z is not tested.  The cell of a coordinate is floor((p - lo) / vs) in float32 with a
 * correctly rounded division (the function of pda_voxelize).  A row joins nothing when a cell lies outside the grid, when x, y
 * or z is NaN, or when its batch index (truncated towards zero) lies outside [0, batch).
 * key = merge_coords: b * gx*gy*gz + cx * gy*gz + cy * gz + cz, pillars b * gx*gy + cx * gy + cy.  The reference computes it
 * in int32 and wraps silently; here batch * cells >= 2^31 is refused before any launch.
 * Outputs, all int32, padded to n rows, zero beyond the live counts:
 *   counts (2) = [n_kept, n_voxels];
 *   point_idx (n): the kept rows in ascending order (points[mask]); "kept position" i below means point_idx[i];
 *   unq_inv (n): for kept position i the rank of its key among the distinct keys in ascending order;
 *   unq_cnt (n): the points of voxel v;  voxel_coords (n, 4): (b, z, y, x), pillars (b, 0, y, x);
 *   seg_start (n + 1), seg_points (n): voxel v holds the kept positions seg_points[seg_start[v] .. seg_start[v + 1]), ascending;
 *   seg_start[n_voxels] = n_kept.
 * workspace: pda_dyn_voxel_workspace_bytes(n, key_bits) bytes, 4-byte aligned, key_bits = the bits of batch * cells - 1
 * (1 .. 31); -1 for bad sizes.  A stable radix sort of (key, kept position), 8 bits a pass, ceil(key_bits / 8) passes.
 * Every grid is sized from n alone; nothing is read back or allocated (graph-capturable); the only atomics are integer adds in
 * LDS, and two runs give the same bits.  n == 0 returns PDA_OK and touches nothing. */
int64_t pda_dyn_voxel_workspace_bytes(int64_t n, int key_bits);
int pda_dyn_voxel_index(const float *points, int64_t n, int columns, const float *range6, const float *voxel_size3,
                        const int32_t *grid3, int batch, int pillars, int32_t *counts, int32_t *point_idx, int32_t *unq_inv,
                        int32_t *unq_cnt, int32_t *voxel_coords, int32_t *seg_start, int32_t *seg_points, void *workspace,
                        pda_stream_t stream);
/* The reductions walk seg_start / seg_points and read the live counts on the device; `rows` is the number of rows the output
 * holds (rows beyond n_voxels are written as zeros; seg_start holds at least rows + 1 entries).  One thread per (voxel, column).
 * pda_dyn_scatter_mean: out[v][f] = (the float32 sum of src[p][f] over the voxel's kept positions p in ascending order) /
 * float32(count): torch_scatter.scatter_mean's sum / count with the order of the sum fixed.  src (>= n_kept, columns).
 * pda_dyn_scatter_max_fwd: out[v][f] = the maximum, arg[v][f] = the lowest kept position that attains it (torch_scatter's CPU
 * rule: an update needs a strictly greater value). */
int pda_dyn_scatter_mean(const float *src, int columns, const int32_t *seg_start, const int32_t *seg_points,
                         const int32_t *counts, int64_t rows, float *out, pda_stream_t stream);
int pda_dyn_scatter_max_fwd(const float *x, int columns, const int32_t *seg_start, const int32_t *seg_points,
                            const int32_t *counts, int64_t rows, float *out, int32_t *arg, pda_stream_t stream);
/* grad_x (rows, columns): grad_x[p][f] = grad_out[v][f] when p == arg[v][f] for v = unq_inv[p], else 0 -- rows that are the
 * argmax of nothing and rows beyond n_kept are written as zeros here.  grad_out, arg (vox_rows, columns).  No atomics. */
int pda_dyn_scatter_max_bwd(const float *grad_out, const int32_t *arg, const int32_t *unq_inv, const int32_t *counts,
                            int64_t rows, int64_t vox_rows, int columns, float *grad_x, pda_stream_t stream);
/* The rows DynamicPillarVFE feeds its first PFN layer, for every kept position i (row r = point_idx[i], voxel v = unq_inv[i]):
 * [points[r, 1:] (absolute_xyz == 1) or points[r, 4:], xyz - mean[v], x - (float32(cx) * vx + offset_x), y - (float32(cy) * vy
 * + offset_y), z - offset_z, (sqrt(fma(z, z, fma(y, y, x*x))) when with_distance == 1)]; mean (>= n_voxels, 3) from
 * pda_dyn_scatter_mean; HOST arrays voxel_size3 and offset3 = float32(v / 2 + lo), computed by the caller in double.
 * out (n, width), width = columns - 1 or columns - 4, + 6, + with_distance; rows beyond n_kept are written as zeros. */
int pda_dyn_pillar_features(const float *points, int64_t n, int columns, const int32_t *point_idx, const int32_t *unq_inv,
                            const int32_t *voxel_coords, const float *mean, const int32_t *counts, const float *voxel_size3,
                            const float *offset3, int absolute_xyz, int with_distance, float *out, pda_stream_t stream);

/* ---- CenterPoint pillar tail (csrc/pillar.hip: the scatter; csrc/center_head.hip: the head) -------------------------------------
 * PointPillarScatter (backbones_2d/map_to_bev/pointpillar_scatter.py) and CenterHead's target assignment, losses and
 * decoding (dense_heads/center_head.py, model_utils/centernet_utils.py, utils/loss_utils.py:395-517).  Every launch goes on
 * `stream`, nothing is allocated, sizes are checked before any pointer is used and an empty problem is PDA_OK and touches
 * nothing.
 *
 * pda_pillar_scatter_fwd: features (n, c) float32, coords (n, 4) int32 (b, z, y, x) -> out (b, c, ny, nx), ZERO-FILLED BY THE
 * CALLER: out[coords[0], :, cell] = features row with cell = c1 + c2 * nx + c3.  A row is skipped when its batch index is
 * outside [0, b) or its cell outside [0, ny * nx); with count != NULL (a device int32) also the rows from *count on (the
 * padded form of pda_dyn_voxel_index).  Two rows on one cell are outside the contract.  pda_pillar_scatter_bwd is the gather
 * of the same cells from grad_out (b, c, ny, nx) into grad_features (n, c), zero for a skipped row; no atomics. */
int pda_pillar_scatter_fwd(const float *features, const int32_t *coords, const int32_t *count, int64_t n, int c, int b, int ny,
                           int nx, float *out, pda_stream_t stream);
int pda_pillar_scatter_bwd(const float *grad_out, const int32_t *coords, const int32_t *count, int64_t n, int c, int b, int ny,
                           int nx, float *grad_features, pda_stream_t stream);
/* CenterHead.assign_targets for b scenes and n_heads heads in one launch, no host read.  gt_boxes (b, m, gt_cols) float32,
 * zero-padded, the label (1-based, 0 = none) in the last column; it is not written.  HOST arrays: head_of_class and
 * local_of_class (num_class + 1, by label; head -1 = no head), head_classes (n_heads) the classes of each head, and per
 * head the DEVICE pointers heatmaps[h] (b, head_classes[h], h, w) float32 ZERO-FILLED BY THE CALLER, target_boxes[h]
 * (b, max_objs, gt_cols) float32, inds[h] and masks[h] (b, max_objs) int64, all three written whole.  Per (scene, head) the
 * rows of the head's classes are compacted in row order; row k of that list is object k; objects from max_objs on are
 * dropped; an object with dx <= 0 or dy <= 0 leaves its slot zero.  Per object every operation is a float32 one:
 * coord = clamp(((x - pcr0) / vs0) / stride, 0, w - 0.5), inds = int(coord_y) * w + int(coord_x), target_boxes =
 * [coord - int(coord) (2), z, log(dims) (3), cos(ry), sin(ry), columns 7..gt_cols-2] with log, cos and sin evaluated in
 * double and rounded once, radius = max(int(gaussian_radius(dx / vs0 / stride, dy / vs1 / stride, gaussian_overlap)),
 * min_radius).  The Gaussian exp(-(i*i + j*j) / (2 sigma^2)), sigma = (2 r + 1) / 6, evaluated in double and rounded, is
 * written over the clipped window with an integer atomicMax on the bit pattern: the result is independent of any order.
 * gaussian2D's eps cut-off cannot fire with this sigma (the corner value is about e^-9) and is left out. */
int pda_center_assign_targets(const float *gt_boxes, int gt_cols, int b, int m, int num_class, int n_heads,
                              const int32_t *head_of_class, const int32_t *local_of_class, const int32_t *head_classes, int h,
                              int w, int max_objs, double pcr0, double pcr1, double vs0, double vs1, double stride,
                              double gaussian_overlap, int min_radius, void *const *heatmaps, void *const *target_boxes,
                              void *const *inds, void *const *masks, pda_stream_t stream);
/* FocalLossCenterNet (neg_loss_cornernet) on pred = clamp(sigmoid(logits), 1e-4, 1 - 1e-4) in one pass and one small second
 * launch: out[0] the loss, out[1] = d loss / d (pos + neg) (-1 / num_pos, or -1 without a cell of heatmap == 1), out[2]
 * num_pos; grad (n) the derivative of (pos + neg) with respect to the logits, zero where the clamp is active; partials:
 * 3 * pda_center_focal_blocks(n) float64 of scratch.  Fixed summation order, no float atomics. */
int64_t pda_center_focal_blocks(int64_t n);
int pda_center_focal_loss(const float *logits, const float *heatmap, int64_t n, float *grad, double *partials, float *out,
                          pda_stream_t stream);
/* out (n) = g (n) * (a[0] * b[0] * c), a and b device scalars: the focal loss's backward. */
int pda_center_scale(const float *g, const float *a, const float *b, float c, int64_t n, float *out, pda_stream_t stream);
/* RegLossCenterNet over the n_maps HEAD_ORDER maps as they are: HOST arrays maps (device pointers, map i (b, channels[i], hw)
 * float32), channels and code_weights (sum of channels <= 16); targets (b, k, code) float32, inds and masks (b, k) int64.
 * Per code column sum |pred * m - target * m| over (b, k), m = mask * not-NaN(target), / max(sum(mask), 1); out =
 * [sum(column * code_weight) * loc_weight, max(sum(mask), 1), the columns (code)].  An entry whose target is NaN
 * contributes 0.  A cell index outside [0, hw) is skipped.  One launch, fixed order.  pda_center_reg_loss_grad adds
 * sign * m * code_weight * loc_weight / num * grad_out[0] into grad_maps (ZERO-FILLED BY THE CALLER) with a float
 * atomicAdd, because two objects can share a cell; the sum depends on the order only from three objects on one cell on. */
int pda_center_reg_loss(const void *const *maps, const int32_t *channels, int n_maps, const float *targets, const int64_t *inds,
                        const int64_t *masks, const float *code_weights, float loc_weight, int b, int k, int64_t hw,
                        float *out, pda_stream_t stream);
int pda_center_reg_loss_grad(const void *const *maps, const int32_t *channels, int n_maps, const float *targets,
                             const int64_t *inds, const int64_t *masks, const float *code_weights, float loc_weight, int b,
                             int k, int64_t hw, const float *fwd_out, const float *grad_out, void *const *grad_maps,
                             pda_stream_t stream);
/* decode_bbox_from_heatmap behind the top-k selection: top_logits (b, k) float32 and top_inds (b, k) int64 into the
 * flattened (n_cls * h * w) heat map of a head; center (b, 2, h, w), center_z (b, 1, h, w), dim (b, 3, h, w), rot (b, 2, h, w),
 * vel (b, 2, h, w) or NULL.  boxes (b, k, 7 or 9) = [(cell_x + center_x) * stride * vs0 + pcr0, y alike, z, exp(dim),
 * atan2(sin, cos), vel] (exp and atan2 in double, rounded once), scores (b, k) = sigmoid(logit), or -inf for a row outside
 * limit_range (HOST, 6) or, with use_thresh, not above score_thresh; labels (b, k) int64 = class_map[class] (HOST, n_cls). */
int pda_center_decode(const float *top_logits, const int64_t *top_inds, const float *center, const float *center_z,
                      const float *dim, const float *rot, const float *vel, int b, int k, int h, int w, int n_cls,
                      const int32_t *class_map, double stride, double vs0, double vs1, double pcr0, double pcr1,
                      const float *limit_range, int use_thresh, double score_thresh, float *boxes, float *scores,
                      int64_t *labels, pda_stream_t stream);

/* ---- PointPillar / anchor heads (csrc/anchor_head.hip; csrc/pillar.hip: pda_pillar_features) ------------------------------------
 * AxisAlignedTargetAssigner.assign_targets, AnchorHeadTemplate's losses and generate_predicted_boxes
 * (dense_heads/anchor_head_template.py, target_assigner/axis_aligned_target_assigner.py, utils/loss_utils.py,
 * utils/box_coder_utils.py ResidualCoder) and the PFN input rows of the hard-voxel PillarVFE (backbones_3d/vfe/pillar_vfe.py).
 * Every launch goes on `stream`, nothing is allocated, sizes are checked before any pointer is used.
 *
 * pda_anchor_assign_targets: all scenes and all anchor classes in two launches (plus two memsets), no host read.
 * gt_boxes (b, m, 8) float32, zero-padded, the 1-based label in the last column; it is not written.  anchors (n_anchors, 7)
 * float32 is the table of one scene, the bits of the head's `anchors` in the order of its targets: every cell of the table
 * holds the classes' anchors class after class, class c owning class_count[c] slots; anchor n belongs to the class that owns
 * slot n % sum(class_count).  HOST arrays per anchor class (n_cls <= 32, at most 64 slots): class_label (1-based, pairwise
 * different), matched, unmatched, class_count.  col_max: (b, m) uint32 of scratch.  Outputs, each written whole:
 * box_cls_labels (b, n_anchors) int32, box_reg_targets (b, n_anchors, 7), reg_weights (b, n_anchors), num_pos (b) int32.
 * Per (scene, class c, anchor a of c):
 *  - the participating gts are the rows whose label equals class_label[c].  The reference trims trailing zero rows and maps
 *    a label-0 row onto the last class; such rows have zero area, therefore IoU 0 with everything, and can never influence a
 *    label or a target, so here a row with label 0 takes part in no class;
 *  - iou = boxes3d_nearest_bev_iou in float32, each operation rounded separately: r = |ry - floor(ry / pi + 0.5) * pi|, dims
 *    swapped when !(r < pi / 4), corners c -+ dim / 2, inter from max / min / clamp_min(., 0), iou = inter /
 *    max(area_a + area_b - inter, 1e-6);
 *  - row_max, row_arg: the maximum over the participating gts and its lowest index; col_max[j]: the maximum over the class's
 *    anchors, an integer atomicMax on the bit pattern (all values >= 0), so it depends on no order; a column maximum of 0
 *    counts as -1 and matches nothing;
 *  - the anchor is forced when iou(a, j) == col_max[j] for some participating j; its gt is then row_arg, not j;
 *  - label = class_label[c] when forced; else 0 when row_max < unmatched[c] or the class has no gt in the scene; else
 *    class_label[c] when row_max >= matched[c]; else -1.  A forced anchor keeps its label below the unmatched threshold;
 *  - positives get ResidualCoder.encode_torch(gt[row_arg], anchor): sizes clamped to 1e-5, sqrt and divisions float32, the
 *    three logs evaluated in double and rounded once; reg_weights 1; every other row is zero; num_pos counts them. */
int pda_anchor_assign_targets(const float *gt_boxes, int gt_cols, int b, int m, const float *anchors, int n_anchors, int n_cls,
                              const int32_t *class_label, const float *matched, const float *unmatched,
                              const int32_t *class_count, uint32_t *col_max, int32_t *box_cls_labels, float *box_reg_targets,
                              float *reg_weights, int32_t *num_pos, pda_stream_t stream);
/* get_cls_layer_loss + get_box_reg_layer_loss in one pass and one small finishing launch.  cls_preds (b, n_anchors,
 * num_class), box_preds (b, n_anchors, 7), dir_cls_preds (b, n_anchors, bins) or NULL, the labels, targets and num_pos of
 * pda_anchor_assign_targets, anchors (n_anchors, 7) for the headings, code_weights HOST (7).  Per scene norm = max(num_pos, 1).
 * cls: SigmoidFocalClassificationLoss (alpha 0.25, gamma 2) on the one-hot of the label (num_class == 1: every positive is
 * class 1), weight (label >= 0) / norm, summed, / b * cls_weight.  loc: add_sin_difference on column 6, WeightedSmoothL1Loss
 * (beta 1/9, code_weights), weight (label > 0) / norm, a NaN target contributes 0, / b * loc_weight.  dir: target bin
 * clamp(floor(limit_period(target[6] + anchor[6] - dir_offset, 0, 2 pi) / (2 pi / bins)), 0, bins - 1) in float32, softmax
 * cross-entropy, weight (label > 0) / norm, / b * dir_weight.  out = [rpn_loss_cls, rpn_loss_loc, rpn_loss_dir, rpn_loss];
 * grad_cls, grad_box, grad_dir (the shapes of the predictions, written whole) hold d rpn_loss / d prediction; partials:
 * 3 * pda_anchor_loss_blocks(b * n_anchors) float64 of scratch, summed in a fixed order; no float atomics.  The backward
 * multiplies the gradients by the incoming scalar with pda_center_scale. */
int64_t pda_anchor_loss_blocks(int64_t n);
int pda_anchor_loss(const float *cls_preds, const float *box_preds, const float *dir_cls_preds, const int32_t *box_cls_labels,
                    const float *box_reg_targets, const int32_t *num_pos, const float *anchors, int b, int n_anchors,
                    int num_class, int bins, const float *code_weights, double cls_weight, double loc_weight, double dir_weight,
                    double dir_offset, float *grad_cls, float *grad_box, float *grad_dir, double *partials, float *out,
                    pda_stream_t stream);
/* generate_predicted_boxes in one launch: batch_box_preds (b, n_anchors, 7) = ResidualCoder.decode_torch(box_preds, anchors)
 * in float32 with exp evaluated in double and rounded once; with dir_cls_preds (b, n_anchors, bins) the heading becomes
 * limit_period(ry - dir_offset, dir_limit_offset, 2 pi / bins) + dir_offset + (2 pi / bins) * argmax(dir), the lowest index
 * on a tie. */
int pda_anchor_decode(const float *box_preds, const float *dir_cls_preds, const float *anchors, int b, int n_anchors, int bins,
                      double dir_offset, double dir_limit_offset, float *batch_box_preds, pda_stream_t stream);
/* AnchorHeadMulti (dense_heads/anchor_head_multi.py, USE_MULTIHEAD): the table is class-major, the reference's
 * cat over the classes of anchors.permute(3, 4, 0, 1, 2, 5).view(-1, 7), so class c owns the class_rows[c] contiguous rows behind
 * those of the classes before it (sum = n_anchors) and classes may differ in stride and in their number of rotations.
 * pda_anchor_multi_assign_targets is pda_anchor_assign_targets with that one difference: every other argument, every output and
 * the per-(scene, class, anchor) rule are the same, and so are the two launches, the integer atomicMax and the untouched
 * gt_boxes.  The class-major table with pda_anchor_decode decodes the concatenated box / direction predictions.
 *
 * pda_anchor_multi_loss: get_cls_layer_loss + get_box_reg_layer_loss of anchor_head_multi.py in one pass and one finishing
 * launch over n_heads <= 32 heads whose predictions are tensors of their own.  HOST arrays per head: cls_preds[h]
 * (b, head_rows[h], head_cols[h]), box_preds[h] (b, head_rows[h], 7), dir_cls_preds[h] (b, head_rows[h], bins) (the array NULL:
 * no direction classifier), the gradients grad_*[h] of the same shapes, written whole; head h owns the head_rows[h] rows of the
 * table behind those of the heads before it (sum = n_anchors); a positive of label l is hot at column l - 1 - head_col_base[h]
 * (SEPARATE_MULTIHEAD: the head's first class; otherwise 0 with head_cols = num_class); num_class == 1: every positive is
 * hot at column 0.  labels, targets, num_pos (of all heads together, the reference's normaliser), anchors, code_weights and
 * the terms are pda_anchor_loss's, each head's sum / b * weight, with two departures the reference makes: the classification
 * weight of a positive is pos_cls_weight / norm and of a negative neg_cls_weight / norm, and the sin difference is taken
 * only behind a direction classifier.  out = [rpn_loss_cls, rpn_loss_loc, rpn_loss_dir, rpn_loss]; partials: 3 *
 * pda_anchor_multi_loss_blocks(b * n_anchors) float64. */
int pda_anchor_multi_assign_targets(const float *gt_boxes, int gt_cols, int b, int m, const float *anchors, int n_anchors,
                                    int n_cls, const int32_t *class_label, const float *matched, const float *unmatched,
                                    const int32_t *class_rows, uint32_t *col_max, int32_t *box_cls_labels,
                                    float *box_reg_targets, float *reg_weights, int32_t *num_pos, pda_stream_t stream);
int64_t pda_anchor_multi_loss_blocks(int64_t n);
int pda_anchor_multi_loss(const float *const *cls_preds, const float *const *box_preds, const float *const *dir_cls_preds,
                          int n_heads, const int32_t *head_rows, const int32_t *head_cols, const int32_t *head_col_base,
                          const int32_t *box_cls_labels, const float *box_reg_targets, const int32_t *num_pos,
                          const float *anchors, int b, int n_anchors, int num_class, int bins, const float *code_weights,
                          double cls_weight, double loc_weight, double dir_weight, double dir_offset, double pos_cls_weight,
                          double neg_cls_weight, float *const *grad_cls, float *const *grad_box, float *const *grad_dir,
                          double *partials, float *out, pda_stream_t stream);
/* The same five entries for ResidualCoder's wider codes (nuscenes_models/cbgs_*_multihead.yaml: code_size 9,
 * encode_angle_by_sincos).  extra = gt_cols - 8 in 0..2 custom columns (velocities) stand behind the heading, sincos is 0 or 1,
 * and a code row holds code = 6 + (sincos ? 2 : 1) + extra columns, 7..10: [x, y, z, log sizes, heading | cos, sin, custom].
 * The anchors stay (n_anchors, 7): the reference pads them with zero columns, so a custom target is the gt's own value and a
 * decoded custom column the code's own.  Every argument not named here, every check and every launch is that of the entry
 * without the suffix, which runs the (code 7, sincos 0, smooth L1) instantiation of the same kernels.
 *  - pda_anchor_assign_targets_coded, pda_anchor_multi_assign_targets_coded: gt_boxes (b, m, gt_cols), the label last; matching
 *    reads columns 0..6 only.  box_reg_targets (b, n_anchors, code): columns 0..5 as before; with sincos columns 6, 7 are
 *    cos(rg) - cos(ra) and sin(rg) - sin(ra), each cosine and sine evaluated in double and rounded once, the difference
 *    float32; without, column 6 is rg - ra; the custom columns carry the gt's bits (a NaN velocity stays NaN).
 *  - pda_anchor_loss_coded, pda_anchor_multi_loss_coded: box_preds, box_reg_targets and grad_box rows are code wide,
 *    code_weights HOST (code).  reg_loss: PDA_REG_SMOOTH_L1 (WeightedSmoothL1Loss, beta 1/9) or PDA_REG_L1 (WeightedL1Loss:
 *    |diff * code_weight| * weight, gradient sign(diff) * code_weight, 0 at diff == 0).  A NaN target contributes 0 to the
 *    loss and the gradient under both.  The sine difference and the direction term read column 6 of a scalar heading only:
 *    sincos with dir_cls_preds != NULL returns 1, and with sincos there is no sine difference.
 *  - pda_anchor_decode_coded: batch_box_preds (b, n_anchors, 7 + extra).  With sincos the heading is
 *    atan2(sin_t + sin(ra), cos_t + cos(ra)): sin(ra), cos(ra) in double and rounded once, the sums float32, the atan2 in
 *    double and rounded once; no direction bins.  Custom columns are t + 0.
 * Out-of-range gt_cols / code, a sincos or reg_loss that is no such value, sincos with dir_cls_preds and null pointers return
 * 1 with pda_last_error() naming the argument, before any pointer is used. */
#define PDA_REG_SMOOTH_L1 0
#define PDA_REG_L1 1
int pda_anchor_assign_targets_coded(const float *gt_boxes, int gt_cols, int sincos, int b, int m, const float *anchors,
                                    int n_anchors, int n_cls, const int32_t *class_label, const float *matched,
                                    const float *unmatched, const int32_t *class_count, uint32_t *col_max,
                                    int32_t *box_cls_labels, float *box_reg_targets, float *reg_weights, int32_t *num_pos,
                                    pda_stream_t stream);
int pda_anchor_multi_assign_targets_coded(const float *gt_boxes, int gt_cols, int sincos, int b, int m, const float *anchors,
                                          int n_anchors, int n_cls, const int32_t *class_label, const float *matched,
                                          const float *unmatched, const int32_t *class_rows, uint32_t *col_max,
                                          int32_t *box_cls_labels, float *box_reg_targets, float *reg_weights, int32_t *num_pos,
                                          pda_stream_t stream);
int pda_anchor_loss_coded(int code, int sincos, int reg_loss, const float *cls_preds, const float *box_preds,
                          const float *dir_cls_preds, const int32_t *box_cls_labels, const float *box_reg_targets,
                          const int32_t *num_pos, const float *anchors, int b, int n_anchors, int num_class, int bins,
                          const float *code_weights, double cls_weight, double loc_weight, double dir_weight, double dir_offset,
                          float *grad_cls, float *grad_box, float *grad_dir, double *partials, float *out, pda_stream_t stream);
int pda_anchor_multi_loss_coded(int code, int sincos, int reg_loss, const float *const *cls_preds, const float *const *box_preds,
                                const float *const *dir_cls_preds, int n_heads, const int32_t *head_rows,
                                const int32_t *head_cols, const int32_t *head_col_base, const int32_t *box_cls_labels,
                                const float *box_reg_targets, const int32_t *num_pos, const float *anchors, int b, int n_anchors,
                                int num_class, int bins, const float *code_weights, double cls_weight, double loc_weight,
                                double dir_weight, double dir_offset, double pos_cls_weight, double neg_cls_weight,
                                float *const *grad_cls, float *const *grad_box, float *const *grad_dir, double *partials,
                                float *out, pda_stream_t stream);
int pda_anchor_decode_coded(int code, int sincos, const float *box_preds, const float *dir_cls_preds, const float *anchors, int b,
                            int n_anchors, int bins, double dir_offset, double dir_limit_offset, float *batch_box_preds,
                            pda_stream_t stream);
/* PillarVFE's PFN input rows: voxels (v, p, c) float32 (c >= 3, padded rows zero), voxel_num_points (v) int32, voxel_coords
 * (v, 4) int32 (b, z, y, x) -> out (v, p, c' ) with c' = (absolute_xyz ? c : c - 3) + 6 + (with_distance ? 1 : 0): [the raw
 * columns (from column 3 on without absolute_xyz), xyz - mean, xyz - cell centre, |xyz|]; rows from num_points on are exactly
 * zero.  The mean is the float32 sum over all p rows IN ROW ORDER divided by num_points; the cell centre is
 * coord * voxel_size3 + offset3 (HOST float32 arrays, offset3 = float32(voxel / 2 + range_lo)), a multiplication and an
 * addition.  One launch, one wave per voxel. */
int pda_pillar_features(const float *voxels, const int32_t *voxel_num_points, const int32_t *voxel_coords, int64_t v, int p,
                        int c, const float *voxel_size3, const float *offset3, int absolute_xyz, int with_distance, float *out,
                        pda_stream_t stream);

/* ---- Sparse 3D convolution (csrc/sparse_conv_index.hip: the index stage; csrc/sparse_conv.hip: the feature kernels) --------------
 * spconv 2.x semantics for SubMConv3d and SparseConv3d (dilation 1) over a sparse tensor of n rows: indices (n, 4) int32
 * (b, z, y, x) in a grid (d, h, w) of `batch` scenes, features (n, C) float32.  Taps are numbered t = (tz * kh + ty) * kw + tx.
 * Every launch goes on `stream`, nothing is allocated or read back, sizes are checked before any pointer is used, and an empty
 * problem (n == 0) is PDA_OK and touches nothing.  batch * d * h * w >= 2^31, for the input or the output grid, is refused
 * before any launch.
 *
 * The index stage reads coordinates only.  stat (2) int32 is written whole: stat[0] the number of output sites (strided form;
 * it keeps counting past cap), stat[1] flags: 1 = two rows share a coordinate, 2 = a row lies outside the grid.  Such rows
 * are outside the contract: the caller reads the flags and refuses the tensor.  Only integer work, the only atomics are integer
 * ones, two runs give the same bits; every grid is sized from n and cap.  workspace: pda_spconv_index_workspace_bytes(n, cap,
 * candidates) bytes, 256-byte aligned; candidates = prod ceil(k_a / s_a), and (n, 0, 1) for the submanifold form; -1 for bad
 * sizes.
 * pda_spconv_index_subm: odd kernel, stride 1: the output sites are the input sites in the input's row order.
 *   nbr_out (n, T): the row at coord_i + (t - centre), or -1 when that site is inactive or outside the grid.  The map a data
 *   gradient needs is nbr_out with the taps mirrored (t -> T - 1 - t).
 * pda_spconv_index_strided: kernel k, stride s, padding p per axis; the output grid is (in + 2p - k) / s + 1 per axis; an output
 *   site is active when an active input site lies in its window.  out_indices (cap, 4): the output sites in ascending linear key
 *   ((b * d' + z) * h' + y) * w' + x; rows from min(stat[0], cap) on are not written.  nbr_out (cap, T): the input row at
 *   o * s - p + t or -1, -1 in the rows from min(stat[0], cap) on.  nbr_in (n, T): the output row that reads input row j through
 *   tap t, or -1. */
int64_t pda_spconv_index_workspace_bytes(int64_t n, int64_t cap, int candidates);
int pda_spconv_index_subm(const int32_t *indices, int64_t n, int batch, int d, int h, int w, int kd, int kh, int kw,
                          int32_t *nbr_out, int32_t *stat, void *workspace, pda_stream_t stream);
int pda_spconv_index_strided(const int32_t *indices, int64_t n, int batch, int d, int h, int w, int kd, int kh, int kw, int sd,
                             int sh, int sw, int pd, int ph, int pw, int64_t cap, int32_t *out_indices, int32_t *nbr_out,
                             int32_t *nbr_in, int32_t *stat, void *workspace, pda_stream_t stream);
/* The counted builds, for padded tensors: n is the CAPACITY of the input and *count_in, a device word, the
 * number of live rows, clipped to [0, n].  Rows from *count_in on take part in nothing and raise no flag, whatever they hold.
 * status is one device word that the build ORs its flags into and never clears: 1 and 2 as above, 4 = more output sites than
 * cap (the cap smallest keys are kept, so the result is still determined).  The strided form writes *count_out = min(found,
 * cap), out_indices (cap, 4) and nbr_out (cap, T) with -1 in the rows from *count_out on, nbr_in (n, T) with -1 in the rows from
 * *count_in on; its first *count_out rows are what pda_spconv_index_strided returns for the live rows alone.  The submanifold
 * form writes nbr_out (n, T), -1 in the rows from *count_in on.  Every grid and the workspace (the same query) depend on n and
 * cap only; nothing is read back. */
int pda_spconv_index_subm_counted(const int32_t *indices, int64_t n, const int32_t *count_in, int batch, int d, int h, int w,
                                  int kd, int kh, int kw, int32_t *nbr_out, int32_t *status, void *workspace,
                                  pda_stream_t stream);
int pda_spconv_index_strided_counted(const int32_t *indices, int64_t n, const int32_t *count_in, int batch, int d, int h, int w,
                                     int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, int64_t cap,
                                     int32_t *out_indices, int32_t *nbr_out, int32_t *nbr_in, int32_t *count_out,
                                     int32_t *status, void *workspace, pda_stream_t stream);
/* The feature kernels: float32 in, float32 accumulate with the exact f32-input MFMA, no float atomics, fixed summation
 * orders.  cin in [1, 128], cout a multiple of 16 up to 128; anything else is refused with a message.
 * pda_spconv_gemm: out[i] = sum_t in[nbr[i][t']] . plane[t] (+ bias), t' = flip ? T - 1 - t : t, a tap with nbr < 0 (or
 *   >= n_src) dropped.  transposed == 0 is the forward: in (n_src, cin), plane (T, pad16(cin), cout) with plane[t][ci][co] =
 *   weight[co][t][ci], out (n_rows, cout), bias (cout) or NULL.  transposed == 1 is the data gradient: in = grad_out
 *   (n_src, cout), plane (T, cout, pad16(cin)) with plane[t][co][ci] = weight[co][t][ci], out = grad_in (n_rows, cin), nbr =
 *   nbr_in (or nbr_out with flip for the submanifold form).  pad16 rounds up to a multiple of 16; the padding is zero.
 * pda_spconv_wgrad: grad_weight (cout, T, cin) [t][ci] = sum_i in[nbr_out[i][t]][ci] * grad_out[i][co], grad_bias (cout) or
 *   NULL the column sums of grad_out (n_out, cout); partial products per (tap, row block) go to the workspace
 *   (pda_spconv_wgrad_workspace_bytes, -1 for bad sizes) and are added in ascending block order. */
int pda_spconv_gemm(const float *in, const int32_t *nbr, const float *plane, const float *bias, float *out, int64_t n_rows,
                    int64_t n_src, int taps, int cin, int cout, int transposed, int flip, pda_stream_t stream);
int64_t pda_spconv_wgrad_workspace_bytes(int64_t n_out, int taps, int cin, int cout);
int pda_spconv_wgrad(const float *in, const float *grad_out, const int32_t *nbr_out, int64_t n_out, int64_t n_in, int taps,
                     int cin, int cout, float *grad_weight, float *grad_bias, void *workspace, pda_stream_t stream);

/* ---- Fused voxel pooling (csrc/voxel_pool.hip): one scale of NeighborVoxelSAModuleMSG after mlps_in, without the grouped
 * (M, C, nsample) tensors.  idx (m, nsample) is pda_stack_voxel_query's output as it stands: GLOBAL rows of xyz, idx[i][0] = -1
 * for an empty ball.  A slot of an empty row, and a slot g outside [0, n), reads nothing and stands for rel = 0, f = 0.
 *   rel[i][s] = xyz[idx[i][s]] - new_xyz[i]  (the float32 difference),  f[i][s][c] = features_in[idx[i][s]][c]
 *   out[i][c] = max_s relu(f[i][s][c] + scale[c] * (w[c] . rel[i][s]) + shift[c]),  arg[i][c] = the first s that attains it
 * c is 32 or 64, nsample in [1, 255]; anything else is refused with a message.
 * pda_voxel_pool_scratch_doubles: the float64 elements the scratch of the two entries below needs (-1 for bad sizes).
 * pda_voxel_pool_moments: sums[9] = sum over all m * nsample slots of [x, y, z, xx, xy, xz, yy, yz, zz] of rel, in float64,
 *   per-workgroup partials added in one fixed order (csrc/loss_sums.h); no atomics.
 * pda_voxel_pool_bwd: with g = grad_out where out > 0 (else 0) and s* = arg: grad_features_in[idx[i][s*]][c] += g by float
 *   atomics (the caller zero-fills it; slots that read nothing add nothing), and sums (5, c) float64 = per channel
 *   [sum g, sum g * (w[c] . rel*), sum g * rel*.x, .y, .z], ordered partials as above. */
int64_t pda_voxel_pool_scratch_doubles(int m, int c, int nsample);
int pda_voxel_pool_moments(const int32_t *idx, const float *xyz, const float *new_xyz, double *scratch, double *sums, int n,
                           int m, int nsample, pda_stream_t stream);
int pda_voxel_pool_fwd(const float *features_in, const int32_t *idx, const float *xyz, const float *new_xyz, const float *w,
                       const float *scale, const float *shift, float *out, uint8_t *arg, int n, int m, int c, int nsample,
                       pda_stream_t stream);
int pda_voxel_pool_bwd(const float *grad_out, const float *out, const uint8_t *arg, const int32_t *idx, const float *xyz,
                       const float *new_xyz, const float *w, float *grad_features_in, double *scratch, double *sums, int n,
                       int m, int c, int nsample, pda_stream_t stream);

/* ---- Fused stacked set abstraction (csrc/stack_sa.hip): one scale of StackSAModuleMSG with two Conv-BN-ReLU layers and a max
 * pool, without the grouped (M, 3 + C_in, nsample) tensor and what follows it.  f (n, c1) = features W1f^T is made by the
 * caller (W1 = [W1x | W1f], xyz first).  idx (m, nsample) is pda_stack_ball_query's output as it stands: indices LOCAL to the
 * scene, idx[i][0] = -1 for an empty ball; the scene starts are derived on the device from the two count vectors (b scenes).
 * A slot of an empty row, and a slot whose index lies outside its scene, reads nothing and stands for rel = 0, f = 0.
 *   rel = xyz[g] - new_xyz[i];  y1[c] = f[g][c] + ((w1x[c][0] rel.x + w1x[c][1] rel.y) + w1x[c][2] rel.z)
 *   z1[c] = max(scale1[c] y1[c] + shift1[c], 0);  y2[d] = fma chain over c ascending of w2[d][c] z1[c]
 * c1 and c2 are 16, 32 or 64, nsample in [1, 255]; anything else is refused with a message.  Nothing is allocated; every sum
 * is float64 from per-workgroup partials added in one fixed order (csrc/loss_sums.h), no float atomics but grad_f's.
 * pda_stack_sa_scratch_doubles: the float64 elements `scratch` of the entries below needs (-1 for bad sizes).
 * pda_stack_sa_moments: sums (2, c1) = per channel [sum y1, sum y1^2] over all m * nsample slots.
 * pda_stack_sa_fwd: u (m, c2) = the largest y2 over the slots where gamma2[d] >= 0, else the smallest; arg (m, c2) the first
 *   slot that attains it; sums (2, c2) = [sum y2, sum y2^2] over all slots.
 * pda_stack_sa_apply: out = max(scale2[d] u + shift2[d], 0).
 * pda_stack_sa_bwd1: dy2[i][s][d] = (s == arg[i][d] ? scale2[d] g[i][d] : 0) - a2[d] - b2[d] y2[i][s][d];
 *   e1 (m, nsample, c1) = (sum_d dy2[d] w2[d][c]) where z1[c] > 0, else 0;
 *   sums = [dW2 transposed (c1, c2): sum dy2[d] z1[c]] [sum e1 (c1)] [sum e1 y1 (c1)].
 * pda_stack_sa_bwd2: dy1 = (scale1[c] e1 - a1[c]) - b1[c] y1 for the slots that read a row g: grad_f[g][c] += dy1 by float
 *   atomics (the caller zero-fills it), sums (3, c1) = sum dy1[c] rel.x, .y, .z. */
int64_t pda_stack_sa_scratch_doubles(int m, int c1, int c2, int nsample);
int pda_stack_sa_moments(const float *f, const float *xyz, const float *new_xyz, const int32_t *xyz_batch_cnt,
                         const int32_t *new_xyz_batch_cnt, const int32_t *idx, const float *w1x, double *scratch, double *sums,
                         int b, int n, int m, int c1, int nsample, pda_stream_t stream);
int pda_stack_sa_fwd(const float *f, const float *xyz, const float *new_xyz, const int32_t *xyz_batch_cnt,
                     const int32_t *new_xyz_batch_cnt, const int32_t *idx, const float *w1x, const float *w2,
                     const float *scale1, const float *shift1, const float *gamma2, float *u, uint8_t *arg, double *scratch,
                     double *sums, int b, int n, int m, int c1, int c2, int nsample, pda_stream_t stream);
int pda_stack_sa_apply(const float *u, const float *scale2, const float *shift2, float *out, int m, int c2, pda_stream_t stream);
int pda_stack_sa_bwd1(const float *f, const float *xyz, const float *new_xyz, const int32_t *xyz_batch_cnt,
                      const int32_t *new_xyz_batch_cnt, const int32_t *idx, const float *w1x, const float *w2,
                      const float *scale1, const float *shift1, const uint8_t *arg, const float *g, const float *scale2,
                      const float *a2, const float *b2, float *e1, double *scratch, double *sums, int b, int n, int m, int c1,
                      int c2, int nsample, pda_stream_t stream);
int pda_stack_sa_bwd2(const float *f, const float *xyz, const float *new_xyz, const int32_t *xyz_batch_cnt,
                      const int32_t *new_xyz_batch_cnt, const int32_t *idx, const float *w1x, const float *e1,
                      const float *scale1, const float *a1, const float *b1, float *grad_f, double *scratch, double *sums, int b,
                      int n, int m, int c1, int nsample, pda_stream_t stream);

/* ---- interpolate_from_bev_features of VoxelSetAbstraction (csrc/stack_sa.hip): bilinear_interpolate_torch of the reference.
 * keypoints (m, 4) [batch, x, y, z] (only the batch column is read), x_idxs / y_idxs (m) the map coordinates the caller
 * derives with the reference's expressions, bev (b, c, h, w) -> out (m, c).  Indices are floored and then clamped, the
 * weights come from the CLAMPED corners (at the border they need not sum to 1), the value is
 * ((Ia wa + Ib wb) + Ic wc) + Id wd in float32.  A batch index outside [0, b) reads nothing (out = 0) and writes nothing.
 * _bwd adds into grad_bev, which the caller zero-fills, with float atomics. */
int pda_bev_interpolate_fwd(const float *keypoints, const float *x_idxs, const float *y_idxs, const float *bev, float *out,
                            int m, int b, int c, int h, int w, pda_stream_t stream);
int pda_bev_interpolate_bwd(const float *keypoints, const float *x_idxs, const float *y_idxs, const float *grad_out,
                            float *grad_bev, int m, int b, int c, int h, int w, pda_stream_t stream);


/* ---- SECONDHead.roi_grid_pool (second_head.py:53-110, csrc/bev_roi_pool.hip): affine_grid + grid_sample (bilinear, zero
 * padding, align_corners=False) over the BEV map for every RoI of the batch in one launch.  bev (b, c, h, w), rois (b, r, 7)
 * [x, y, z, dx, dy, dz, ry] -> out (b * r, c, g, g).  float32 throughout; with x1 = (x - dx/2 - min_x) / cell_x,
 * x2 = (x + dx/2 - min_x) / cell_x (y likewise) theta is the reference's t0..t5 = (x2-x1)/(w-1) cos, (x2-x1)/(w-1) (-sin),
 * (x1+x2-w+1)/(w-1), (y2-y1)/(h-1) sin, (y2-y1)/(h-1) cos, (y1+y2-h+1)/(h-1); for grid row i, column j: u = (2j+1)/g - 1,
 * v = (2i+1)/g - 1, gx = t0 u + t1 v + t2, gy = t3 u + t4 v + t5, ix = ((gx+1) w - 1)/2, iy = ((gy+1) h - 1)/2, corners at
 * floor and floor + 1 with weights from the unclamped position, a corner outside the map contributing nothing.  A position
 * that is not finite or lies outside [-1, w) x [-1, h) reads nothing and gives 0 (csrc/bev_roi_grid.h).  cell_x / cell_y =
 * VOXEL_SIZE * DOWNSAMPLE_RATIO.  g in 1..16, c >= 1, r <= 4096, b <= 65535, h and w >= 2; empty b or r returns at once.
 * No backward: the reference detaches the map. */
int pda_bev_roi_grid_pool(const float *bev, const float *rois, float *out, int b, int r, int c, int h, int w, int g,
                          float min_x, float min_y, float cell_x, float cell_y, pda_stream_t stream);

/* ---- PointRCNNHead.roipool3d_gpu (pointrcnn_head.py:85-130, csrc/roi_pool.hip): the RoI head's input in one launch.
 * xyz (B,N,3), scores (B,N), feat (B,N,C), rois (B,M,7) NOT enlarged, extra: 3 host floats (POOL_EXTRA_WIDTH) ->
 * pooled (B,M,S,5+C) and empty_flag (B,M) int32, both written in full (the caller fills nothing).
 * Selection: the test and the slot order of pda_roipoint_pool3d_fwd on the RoI with extra[k] added to its three extents in
 * float32 (box_utils.enlarge_box3d): the first S points inside in ascending index, slot k >= cnt repeating slot k % cnt.
 * Row of slot k for point p: [x', y', z', scores[p], |xyz[p]| / depth_normalizer - 0.5, feat[p][0..C)] with
 * (dx, dy, dz) = xyz[p] - roi[0:3], cosa = cosf(-roi[6]), sina = sinf(-roi[6]) taken once per RoI,
 * x' = dx * cosa + dy * (-sina), y' = dx * sina + dy * cosa, z' = dz, |p| = sqrtf((x x + y y) + z z); float32, no FMA.
 * A RoI that holds no point has empty_flag 1 and an all-zero block.  So has a row with a value that is not finite: it is
 * recognised on its bit pattern and reaches neither the box test nor cosf / sinf.  points == 0 makes every RoI empty.
 * S in 1..15360, B <= 65535, C >= 0; B == 0 or M == 0 returns at once and touches nothing.  No backward: the reference
 * pools under no_grad.  Two runs give the same bits. */
int pda_roipoint_pool3d_canonical_fwd(const float *xyz, const float *scores, const float *feat, const float *rois,
                                      const float *extra, float depth_normalizer, float *pooled, int32_t *empty_flag,
                                      int batch, int points, int boxes, int channels, int sampled, pda_stream_t stream);

/* ---- Part-A2 (csrc/parta2.hip): the point head's targets and part loss.
 * pda_part_assign_targets: PointHeadTemplate.assign_stack_targets(set_ignore_flag=True, ret_part_labels=True)
 *   (point_head_template.py:49-129) for a ragged stacked point set in one launch.  points (n_points, 4) [batch, x, y, z], any
 *   number of rows per scene in any order; gt_boxes (b, t, 8) [x, y, z, dx, dy, dz, heading, class]; extra_width: 3 host floats
 *   -> labels (n_points) int64 and part_labels (n_points, 3), every entry written.  The box test is pda_points_in_boxes's
 *   (margin 1e-5, lowest box index first); a point inside a box gets 1 (single_class) or the box's class, and
 *   part = rotate_z(p - centre, -heading) / (dx, dy, dz) + 0.5 in float32 (cosf / sinf of the negated heading, no FMA); a point
 *   inside none but inside a box enlarged by extra_width (float32 additions to the extents) gets -1; everything else 0; part
 *   labels are 0 wherever the label is not positive.  A batch value that is not a number, not an integer or outside [0, b)
 *   names no scene: label 0.  points and gt_boxes 16-byte aligned.
 * pda_part_loss: get_part_layer_loss (:157-170).  logits, part_labels (n_points, 3), labels (n_points) int64 ->
 *   out[0] = weight * sum over rows with label > 0 and their 3 columns of bce / (3 * max(1, #pos)), out[1] = weight / (3 *
 *   max(1, #pos)), out[2] = #pos; grad (n_points, 3) = d bce / d logit, zeros in the other rows, so that the logit gradient is
 *   out[1] * grad.  bce = -(t * max(log p, -100) + (1 - t) * max(log(1 - p), -100)), p = sigmoid(logit), evaluated in float64 per
 *   element; the labels are taken as they are.  partials: 2 * pda_part_loss_blocks(n_points) doubles (-1 for a bad size); sums
 *   in float64 in one fixed order, no float atomics, nothing read back. */
int pda_part_assign_targets(const float *points, const float *gt_boxes, const float *extra_width, int64_t *labels,
                            float *part_labels, int64_t n_points, int b, int t, int single_class, pda_stream_t stream);
int64_t pda_part_loss_blocks(int64_t n_points);
int pda_part_loss(const float *logits, const float *part_labels, const int64_t *labels, double weight, float *grad,
                  double *partials, float *out, int64_t n_points, pda_stream_t stream);

/* The input stage of PartA2FCHead (partA2_head.py:104-197; csrc/parta2.hip) for the whole batch: scene segments, ONE collection
 * pass, both poolings and the sparse rows of the live voxels.  rois (b * rois_per_scene, 7), point_coords (n_points, 4)
 * [batch, x, y, z] SCENE-MAJOR, out the pool size (1..16: out^3 voxel counters live in LDS), k_slots MAX_POINTS_PER_VOXEL;
 * rois_total * out^3 < 2^31.  Integer work decides every position: two runs give the same bits.
 * pda_parta2_pool_segments: seg (b + 1) int32, seg[s] = the first row whose batch value is not below s.  flag, when given (one
 *   int32, zeroed by the caller), gets bit 0 set if the batch column is not ascending or holds a value that names no scene.
 * pda_parta2_pool_collect: table (rois_total, out^3, k_slots) int32, NOT filled by the caller: slot 0 of every voxel is written
 *   (the number of points kept, at most k_slots - 1) and slots 1..count hold the first points of the RoI's scene that fall into
 *   the voxel, as GLOBAL rows in ascending order -- the rules of pda_roiaware_pool3d_fwd's collection (csrc/roi_pool_core.h).
 * pda_parta2_pool_sparsify: part channels of point p: part_src[p * src_stride + src_offset + (0..2)] where scores[p] >= thresh
 *   (more exactly: not below it) and 0 elsewhere, and scores[p]; a voxel's four values are their float32 sums in slot order over
 *   (float)count, as pool_method avg gives them.  A voxel is live iff ((v0 + v1) + v2) + v3 in float32 is not +-0.  Writes
 *   *n_live and, for the live voxels in ascending (roi, x, y, z): coords (.., 4) int32 [roi, x, y, z], part_rows (.., 4),
 *   live_vox (..) = roi * out^3 + (x * out + y) * out + z.  The three buffers hold rois_total * out^3 rows (the worst case);
 *   rows from *n_live on are not written.  workspace: pda_parta2_pool_workspace_bytes (-1 for bad sizes), 16-byte aligned.
 * pda_parta2_pool_features: feat_rows (.., channels) = the largest point_features[p][c] over the slots of live voxel e (ties keep
 *   the lower slot, NaN never wins, 0 when nothing wins) and arg_rows its row or -1, as pool_method max; *n_live is read on the
 *   device and the rows from it on are not written.
 * pda_parta2_pool_bwd: grad_features[arg_rows[e][c]][c] += grad_feat_rows[e][c] and, for ch < 3 and every slot p of live voxel e
 *   with scores[p] >= thresh, grad_offset[p][ch] += grad_part_rows[e][ch] / count, both with float atomics into buffers the
 *   caller zero-filled ((n_points, channels) and (n_points, 3)); either gradient may be NULL.  n_live is the host's count. */
int64_t pda_parta2_pool_workspace_bytes(int64_t rois_total, int out);
int pda_parta2_pool_segments(const float *point_coords, int64_t n_points, int b, int32_t *seg, int32_t *flag, pda_stream_t stream);
int pda_parta2_pool_collect(const float *rois, const float *point_coords, const int32_t *seg, int32_t *table, int b,
                            int rois_per_scene, int64_t n_points, int out, int k_slots, pda_stream_t stream);
int pda_parta2_pool_sparsify(const int32_t *table, const float *part_src, int src_stride, int src_offset, const float *scores,
                             float thresh, void *workspace, int32_t *n_live, int32_t *coords, float *part_rows, int32_t *live_vox,
                             int64_t rois_total, int64_t n_points, int out, int k_slots, pda_stream_t stream);
int pda_parta2_pool_features(const float *point_features, const int32_t *table, const int32_t *live_vox, const int32_t *n_live,
                             float *feat_rows, int32_t *arg_rows, int64_t rois_total, int64_t n_points, int channels, int out,
                             int k_slots, pda_stream_t stream);
int pda_parta2_pool_bwd(const int32_t *table, const int32_t *live_vox, const int32_t *arg_rows, const float *scores, float thresh,
                        const float *grad_part_rows, const float *grad_feat_rows, float *grad_offset, float *grad_features,
                        int64_t n_live, int64_t n_points, int channels, int k_slots, pda_stream_t stream);

/* ---- PV-RCNN++ (csrc/spc_sample.hip).
 * pda_roi_point_filter: sample_points_with_roi (voxel_set_abstraction.py:45-75) for a stacked point set and, with
 *   num_sectors > 0, the sector index of sector_fps (:88-90), in one launch and without an n x m tensor.  points (n, 3) ordered by
 *   scene, point_cnt (b) int32 on the device, rois (b, m, roi_channels >= 6) [x, y, z, dx, dy, dz, ...]; ALL m rows of a scene take
 *   part, zero rows included.  float32, no FMA: d = sqrtf((dx dx + dy dy) + dz dz) to every centre, the nearest RoI is the one of
 *   the lowest index among equal distances, half = sqrtf of the same sum over (dims / 2), and mask[p] = d < half + radius.
 *   keys[p] = scene * (num_sectors + 1) + sector with sector = clamp(floorf((atan2f(y, x) + (float)pi) / (float)(2 pi /
 *   num_sectors)), 0, num_sectors) for a kept point and num_sectors for one that is not; keys may be NULL when num_sectors is 0.
 *   Rows past the sum of the counts are not written (the caller fills mask and keys).  b <= 1024; n == 0 or m == 0 returns PDA_OK with nothing written.
 * pda_vector_interp_fwd: the rows of VectorPoolLocalInterpolateModule.forward (pointnet2_modules.py:220-238) without an MLP.
 *   dist, idx (m, g, 3) as pda_stack_three_nn_by_local_idxs leaves them after the caller's sqrt (idx GLOBAL rows of the support
 *   set, idx[.][.][0] == -1 for a cell without neighbour), support_xyz (n, 3), support_features (n, c), grid_centers (m, g, 3) ->
 *   out (m, g * (c + 9)), every element written once: per cell [sum_k w_k features[idx_k] (c) | grid centre - support_xyz[idx_k]
 *   for k = 0, 1, 2 (9)] with r_k = 1 / (dist_k + 1e-8), w_k = r_k / max((r_0 + r_1) + r_2, 1e-8) and the blend evaluated as
 *   pda_stack_three_interpolate evaluates it; zeros for a cell whose idx holds a value outside [0, n).
 * pda_vector_interp_bwd: grad_out (m, g * (c + 9)) is read in place (the nine coordinate columns of a cell are skipped);
 *   grad_support_features[idx_k][ch] += grad_out[cell][ch] * w_k with float atomics into the (n, c) buffer the caller zero-filled,
 *   as pda_stack_three_interpolate_grad does.  Coordinates and grid centres get no gradient. */
int pda_roi_point_filter(const float *points, const int32_t *point_cnt, const float *rois, float radius, uint8_t *mask,
                         int32_t *keys, int64_t n, int b, int m, int roi_channels, int num_sectors, pda_stream_t stream);
int pda_vector_interp_fwd(const float *dist, const int32_t *idx, const float *support_xyz, const float *support_features,
                          const float *grid_centers, float *out, int m, int g, int n, int c, pda_stream_t stream);
int pda_vector_interp_bwd(const float *grad_out, const float *dist, const int32_t *idx, float *grad_support_features, int m,
                          int g, int n, int c, pda_stream_t stream);

/* ---- CaDDN: FrustumToVoxel over the factors of the frustum tensor, and DDNLoss (csrc/frustum_sample.hip) ----------------
 * The reference multiplies softmax(depth_logits)[:, :-1] (B,D,Hf,Wf) into the image features (B,C,Hf,Wf), builds a
 * (B,X,Y,Z,3) grid and calls a 5-D grid_sample.  The trilinear sample of an outer product factorises, so neither the
 * (B,C,D,Hf,Wf) tensor nor the grid exists here:
 *   out[b,c,k,j,i] = sum over the 4 pixel corners (v',u') of  w_uv(v',u') * (sum over the 2 depth corners d' of
 *                    w_d(d') * prob[b,d',v',u']) * feat[b,c,v',u'],          a corner outside the volume contributes 0.
 * Per voxel (i,j,k) of the (gx,gy,gz) grid, in float32:
 *   T = lidar_to_cam[b] @ [[sx,0,0,minx],[0,sy,0,miny],[0,0,sz,minz],[0,0,0,1]]   (voxel_size s, pc_min; multiplied first)
 *   cam = T[:3] @ [i+.5, j+.5, k+.5, 1];  t = cam_to_img[b] @ [cam, 1];  s = |t2| > 1e-8 ? 1/t2 : 1;  (u,v) = (t0,t1) * s
 *   depth = t2 - cam_to_img[b][2][3];  d = the continuous bin index of depth:
 *     mode 0 UD (depth - depth_min) / ((depth_max - depth_min) / D);  mode 1 LID -0.5 + 0.5 sqrt(1 + 8 (depth - depth_min) / bs),
 *     bs = 2 (depth_max - depth_min) / (D (1 + D));  mode 2 SID D (log(1 + depth) - log(1 + depth_min)) / (log(1 + depth_max) -
 *     log(1 + depth_min))
 *   (u,v,d) / (W_img - 1, H_img - 1, D - 1) * 2 - 1 with image_hw = [H_img, W_img] read on the device (the ORIGINAL image
 *   size); a coordinate that is not finite becomes -2; then ((x + 1) * size - 1) / 2 against (wf, hf, d), floor, the two
 *   corners and weights per axis (grid_sample, align_corners=False, zero padding).
 * feat (B,C,Hf,Wf), prob (B,D,Hf,Wf), lidar_to_cam (B,4,4), cam_to_img (B,3,4), image_hw (2) on the device; pc_min and
 * voxel_size: 3 host floats each.  out (B,C,gz,gy,gx) is written in full.  Any c >= 1.
 * pda_frustum_sample_bwd recomputes the corners: grad_feat and grad_prob, both zero-filled by the caller, are accumulated
 * with float atomics after the lanes of a 16-lane row that hit the same cell have been added up. */
int pda_frustum_sample_fwd(const float *feat, const float *prob, const float *lidar_to_cam, const float *cam_to_img,
                           const float *image_hw, float *out, int b, int c, int d, int hf, int wf, int gx, int gy, int gz,
                           const float *pc_min, const float *voxel_size, int mode, float depth_min, float depth_max,
                           pda_stream_t stream);
int pda_frustum_sample_bwd(const float *grad_out, const float *feat, const float *prob, const float *lidar_to_cam,
                           const float *cam_to_img, const float *image_hw, float *grad_feat, float *grad_prob, int b, int c,
                           int d, int hf, int wf, int gx, int gy, int gz, const float *pc_min, const float *voxel_size,
                           int mode, float depth_min, float depth_max, pda_stream_t stream);
/* DDNLoss in one pass over logits (B, num_bins + 1, H, W): per pixel the target bin of depth_maps (B,H,W) (the index above,
 * truncated; below 0, above num_bins or not finite -> num_bins), the focal term -alpha (1 - p_t)^gamma log_softmax(x)_t, and
 * the weight fg_weight if the pixel (v,u) lies in any [floor(u1/f), ceil(u2/f)) x [floor(v1/f), ceil(v2/f)) of boxes2d
 * (B,N,4) [u1,v1,u2,v2] (read only; f = downsample), else bg_weight.  out3 = [loss, fg_loss, bg_loss] float32 with
 * fg/bg_loss = the float64 sum of the weighted terms / (B H W), loss = weight (fg_loss + bg_loss); grad_logits = d loss /
 * d logits.  partials: 2 * pda_ddn_loss_blocks(B H W) doubles of scratch. */
int64_t pda_ddn_loss_blocks(int64_t pixels);
int pda_ddn_loss_fwd_bwd(const float *logits, const float *depth_maps, const float *boxes2d, float *grad_logits,
                         double *partials, float *out3, int b, int num_bins, int h, int w, int n_boxes, int mode,
                         float depth_min, float depth_max, float downsample, double alpha, double gamma, double fg_weight,
                         double bg_weight, double weight, pda_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
