// Launchers of the temporal-head training kernels (train.hip): bi-GRU forward with saved gates, max-over-time with
// argmax, softmax cross-entropy, the backward passes and the SGD update.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tennis_hip.h"
int launch_pool_max_arg(const float *x, int B, int T, int F, float *y, int32_t *arg, hipStream_t s);
int launch_softmax_ce(const float *logits, const int32_t *labels, int B, int C, float *loss, float *dlogits,
                      hipStream_t s);
int launch_dense_bwd(const float *dlogits, const float *pooled, const float *wd, int B, int C, int K, float *dwd,
                     float *dbd, float *dpooled, hipStream_t s);
int launch_scatter_pool_grad(const float *dpooled, const int32_t *arg, int B, int T, int F, float *dseq, hipStream_t s);
// BPTT of launch_rnn_recurrent's recurrence from its seq and save (rnn_bptt.hip): dgi [B*T][dirs*gates*H], hprev [dirs][B*T][H]; GRU
// also dgh (its candidate block differs from dgi's), LSTM ignores dgh - one pre-activation gradient feeds both branches.  valid_len
// [B] or null: steps >= valid_len never ran; dh_last / dc_last [dirs][B][H] or null: d loss / d final state (GRU ignores dc_last).
int launch_rnn_bptt(int gates, const float *seq, const float *save, const float *dseq, const float *wh, float *dgi, float *dgh,
                    float *hprev, int B, int T, int H, hipStream_t s, int dirs = 2, const int32_t *valid_len = nullptr,
                    const float *dh_last = nullptr, const float *dc_last = nullptr);
int launch_gemm_tn_f32(const float *A, int lda, const float *Bm, int ldb, float *Cm, int ldc, int M, int N, int K,
                       hipStream_t s, float *workspace = nullptr, long workspace_floats = 0);   // workspace: enables split-K
// ... with B -> relu(B * bsc[n] + bsh[n]) applied while the operand is staged
int launch_gemm_tn_f32_bnrelu(const float *A, int lda, const float *Bm, int ldb, const float *bsc, const float *bsh, float *Cm, int ldc,
                              int M, int N, int K, hipStream_t s, float *workspace = nullptr, long workspace_floats = 0);
// ... with the B operand gathered from a table: row k of B is table + (long)clamp(rows[k], 0, n_rows - 1) * ld (rows: K int32,
// DEVICE).  Un-split only; equals launch_gemm_tn_f32 (no workspace) on the materialised B bit for bit.
int launch_gemm_tn_f32_rows(const float *A, int lda, const float *table, int ld, const int32_t *rows, int n_rows, float *Cm, int ldc,
                            int M, int N, int K, hipStream_t s);
// ... for ragged clips: rows[k] < 0 is a row of zeros, rows[k] >= n_rows clamps to the last row; equals launch_gemm_tn_f32 (no
// workspace) on the zero-padded materialised B bit for bit.  Pad rows are staged, not skipped: the k-tiles keep their members.
int launch_gemm_tn_f32_padrows(const float *A, int lda, const float *table, int ld, const int32_t *rows, int n_rows, float *Cm, int ldc,
                               int M, int N, int K, hipStream_t s);
// C (M, N; row stride ldc) (+)= A (M, K; row stride lda) B (K, N; row stride ldb), both row-major (gemm_nn.hip)
int launch_gemm_nn_f32(const float *A, int lda, const float *Bm, int ldb, float *Cm, int ldc, int M, int N, int K, int accumulate,
                       hipStream_t s);
int launch_colsum_f32(const float *A, int lda, int rows, int cols, float *out, hipStream_t s);
// scale non-null (both updates): the clipped form, on *scale * g - the scale of a clip record that launch_grad_sumsq filled on the
// same stream; null: the un-clipped kernel, which never sees the pointer's target
int launch_sgd_momentum(float *w, const float *g, float *mom, long n, float lr, float momentum, float wd,
                        float rescale, hipStream_t s, const float *scale = nullptr);
// MXNet Adam (gluon.Trainer 'adam', reference train_gnmt.py:310,337): step = the 1-based update count, its bias correction folded
// into the rate; no weight decay, rescale_grad 1.  Shared by the captioner's parameters (captioner_train.hip) and the backbone's (finetune.hip).
int launch_adam(float *w, const float *g, float *m, float *v, long n, float lr, float beta1, float beta2, float epsilon, long step,
                hipStream_t s, const float *scale = nullptr);
// The device record of a handle's clipping: what grad_sumsq_finalize_kernel writes and the clipped update kernels read (scale)
struct tn_clip_record {
  double sumsq;        // the sum of squares of the last reduction
  float norm, scale;   // of the last reduction
  long long clipped;   // reductions with scale < 1 since the record was zeroed
};
// Global-norm clipping, gluon.utils.clip_global_norm [EXT]: the two-stage, bit-deterministic sum of squares of the segments
// (a, na) and (b, nb) (either may be empty; 4-byte aligned, any count) and the record norm = |rescale| sqrt(sum),
// scale = min(1, max_norm / (norm + 1e-8)), clipped += scale < 1.  partials: TN_GRAD_SUMSQ_GRID floats.  No host synchronisation.
int launch_grad_sumsq(const float *a, long na, const float *b, long nb, float rescale, float max_norm, float *partials,
                      tn_clip_record *rec, hipStream_t s);
// y (B, T, frame_floats) = x with zeros in the frame slots t >= valid_len[b]: what Pad() leaves behind a clip's valid length
int launch_stage_frames(const float *x, const int32_t *valid_len, int B, int T, long frame_floats, float *y, hipStream_t s);
int launch_transpose_f32(const float *src, int rows, int cols, float *dst, hipStream_t s);
// Training-mode BatchNorm of the fine-tuning step (finetune.hip) on an (M, C) matrix of row stride ld: batch mean and biased
// variance; y (M, C contiguous) = relu(gamma (x - mean) / sqrt(var + eps) + beta); its backward from dy (M, C contiguous) into
// dgamma, dbeta and dx (row stride ldd, assigned or accumulated).  ws: ft_bn_ws_floats(M, C) floats.
long ft_bn_ws_floats(long M, int C);
int launch_ft_bn_stats(const float *x, int ld, long M, int C, float *ws, float *mean, float *var, hipStream_t s);
int launch_ft_bn_relu(const float *x, int ld, long M, int C, const float *mean, const float *var, const float *gamma, const float *beta,
                      float *y, hipStream_t s);
int launch_ft_bn_backward(const float *dy, const float *x, int ld, long M, int C, const float *mean, const float *var, const float *gamma,
                          const float *beta, float *ws, float *dgamma, float *dbeta, float *dx, int ldd, int accumulate, hipStream_t s);
// The step's other operators (finetune.hip), NHWC fp32; what the step calls and what the tn_dbg_ft_* hooks run.
// im2col7: 7x7 stride 2 pad 3 of x (B, H, W, 3), H and W even -> col (B H/2 W/2, 147), columns (ky, kx, c).
// im2col3: 3x3 pad 1 of a (B, H, W, C), C % 4 == 0, 16-byte aligned -> col (B H W, 9 C), columns (ky, kx, c); sc / sh non-null: the
// source goes through relu(a sc[c] + sh[c]) first (the padding stays 0).  col2im3: its adjoint, dcol (B H W, 9 C) -> da (B, H, W, C).
// maxpool: 3x3 stride 2 pad 1 (padding never wins) of a (B, H, W, C), H and W even -> y (B H/2 W/2 rows of stride ldy); its gradient
// from dy (rows of stride ldy) goes to the first maximum of a window in (ky, kx) order -> da contiguous.  avgpool2: 2x2 stride 2, the
// same layouts.  gap: mean over the P pixels of a frame, a (B, P, C) -> f (B, C); gradient da = df / P.
// bn_fold: sc = gamma / sqrt(var + 1e-5), sh = beta - mean sc.  bn_running: running = 0.9 running + 0.1 batch, in place.
int launch_ft_im2col7(const float *x, int B, int H, int W, float *col, hipStream_t s);
int launch_ft_im2col3(const float *a, int B, int H, int W, int C, float *col, const float *sc, const float *sh, hipStream_t s);
int launch_ft_col2im3(const float *dcol, int B, int H, int W, int C, float *da, hipStream_t s);
int launch_ft_maxpool(const float *a, int B, int H, int W, int C, float *y, int ldy, hipStream_t s);
int launch_ft_maxpool_bwd(const float *a, const float *dy, int ldy, int B, int H, int W, int C, float *da, hipStream_t s);
int launch_ft_avgpool2(const float *z, int B, int H, int W, int C, float *y, int ldy, hipStream_t s);
int launch_ft_avgpool2_bwd(const float *dy, int ldy, int B, int H, int W, int C, float *dz, hipStream_t s);
int launch_ft_gap(const float *a, int B, int P, int C, float *f, hipStream_t s);
int launch_ft_gap_bwd(const float *df, int B, int P, int C, float *da, hipStream_t s);
int launch_ft_bn_fold(const float *mean, const float *var, const float *gamma, const float *beta, int C, float *sc, float *sh, hipStream_t s);
int launch_ft_bn_running(float *rmean, float *rvar, const float *mean, const float *var, int C, hipStream_t s);
// The fine-tuning step in parts (finetune.hip), what tn_finetune_forward_backward chains and the two frame-trained steps (train_steps.hip) drive.
// ft_create: the table of param_table.h::ft_param_table, loaded, uploaded, then the workspaces; dense_prefix NULL builds the backbone
// alone (no classifier; classes ignored); fit_frames non-NULL: first compare the
// memory batch frames need with what the device has free, and on a shortfall return TN_ERR_NOMEM with *fit_frames = the frames
// that would fit.  ft_forward_features: training-mode forward of x (n, H, W, 3) -> ft_features (n, ft_feature_dim), batch
// statistics kept; ft_backward_features: from ft_feature_grad (n, ft_feature_dim) every backbone gradient, assigned;
// ft_update_running: running = 0.9 running + 0.1 batch for every BatchNorm.
// n: the frames of this step, 1 <= n <= ft_capacity (the batch the handle was created for).  Every row count, statistics divisor
// and launch shape follows n alone, so a step of n frames is bit-identical on any handle that holds them; the backward's n must
// be the forward's.  ft_enable_adam: the second-moment buffer (once, at creation); ft_adam_step: launch_adam on the trainable
// parameters, the momentum buffer as the first moment (the running statistics are no parameters and are not touched).
int ft_create(tn_ctx *ctx, const tn_param *params, int n_params, const char *backbone_prefix, const char *dense_prefix, int height,
              int width, int classes, int batch, tn_finetune **out, long *fit_frames);
int ft_forward_features(tn_finetune *f, const float *x, int n);
int ft_backward_features(tn_finetune *f, int n);
int ft_enable_adam(tn_finetune *f);
int ft_adam_step(tn_finetune *f, float lr, float beta1, float beta2, float epsilon, long step, const float *scale = nullptr);
// tn_finetune_sgd_step's update alone (scale: launch_sgd_momentum's), for the CNN-RNN step, whose one norm spans both parts
int ft_sgd_update(tn_finetune *f, float lr, float momentum, float wd, float rescale_grad, const float *scale);
float *ft_frame_staging(tn_finetune *f);      // (capacity, H, W, 3) floats of the handle's own, for a caller that stages its frames
void ft_update_running(tn_finetune *f);
float *ft_features(tn_finetune *f);
float *ft_feature_grad(tn_finetune *f);
int ft_feature_dim(tn_finetune *f);
// The captioner's training step (captioner_train.hip), what tn_gnmt_trainer_forward_backward runs.  dsrc non-null: also the gradient of
// the loss with respect to src, (batch * steps, input_size) of row stride ldd, assigned; rows at or past src_valid_len[b] are 0.
int gnmt_trainer_step(tn_gnmt_trainer *t, const float *src, const int32_t *src_valid_len, const int32_t *tgt, int ld,
                      const int32_t *tgt_valid_len, int batch, int steps, int tgt_len, float *loss, float *logits_out, float *dsrc, int ldd);
// scale: launch_adam's - the frame-mode handle reduces once over both parts and hands the one scale to both updates
int gnmt_trainer_adam(tn_gnmt_trainer *t, float lr, float beta1, float beta2, float epsilon, long step, const float *scale = nullptr);
