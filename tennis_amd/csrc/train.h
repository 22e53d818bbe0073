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
int launch_gru_train_bwd(const float *seq, const float *gates, const float *dseq, const float *wh, float *dgi,
                         float *dgh, float *hprev, int B, int T, int H, hipStream_t s, int dirs = 2,
                         const int32_t *valid_len = nullptr, const float *dh_last = nullptr);
int launch_lstm_train_bwd(const float *seq, const float *gates, const float *dseq, const float *wh, float *dgi,
                          float *hprev, int B, int T, int H, hipStream_t s, int dirs = 2,
                          const int32_t *valid_len = nullptr, const float *dh_last = nullptr, const float *dc_last = nullptr);
int launch_gemm_tn_f32(const float *A, int lda, const float *Bm, int ldb, float *Cm, int ldc, int M, int N, int K,
                       hipStream_t s, float *workspace = nullptr, long workspace_floats = 0);   // workspace: enables split-K
// ... with B -> relu(B * bsc[n] + bsh[n]) applied while the operand is staged
int launch_gemm_tn_f32_bnrelu(const float *A, int lda, const float *Bm, int ldb, const float *bsc, const float *bsh, float *Cm, int ldc,
                              int M, int N, int K, hipStream_t s, float *workspace = nullptr, long workspace_floats = 0);
// C (M, N; row stride ldc) (+)= A (M, K; row stride lda) B (K, N; row stride ldb), both row-major (gemm_nn.hip)
int launch_gemm_nn_f32(const float *A, int lda, const float *Bm, int ldb, float *Cm, int ldc, int M, int N, int K, int accumulate,
                       hipStream_t s);
int launch_colsum_f32(const float *A, int lda, int rows, int cols, float *out, hipStream_t s);
int launch_sgd_momentum(float *w, const float *g, float *mom, long n, float lr, float momentum, float wd,
                        float rescale, hipStream_t s);
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
// The fine-tuning step in parts (finetune.hip), what tn_finetune_forward_backward chains and the CNN-RNN step (api.hip) drives.
// ft_create: dense_prefix NULL builds the backbone alone (no classifier; classes ignored); fit_frames non-NULL: first compare the
// memory batch frames need with what the device has free, and on a shortfall return TN_ERR_NOMEM with *fit_frames = the frames
// that would fit.  ft_forward_features: training-mode forward of x (B, H, W, 3) -> ft_features (B, ft_feature_dim), batch
// statistics kept; ft_backward_features: from ft_feature_grad (B, ft_feature_dim) every backbone gradient, assigned;
// ft_update_running: running = 0.9 running + 0.1 batch for every BatchNorm.
int ft_create(tn_ctx *ctx, const tn_param *params, int n_params, const char *backbone_prefix, const char *dense_prefix, int height,
              int width, int classes, int batch, tn_finetune **out, long *fit_frames);
int ft_forward_features(tn_finetune *f, const float *x);
int ft_backward_features(tn_finetune *f);
void ft_update_running(tn_finetune *f);
float *ft_features(tn_finetune *f);
float *ft_feature_grad(tn_finetune *f);
int ft_feature_dim(tn_finetune *f);
int ft_param_buffers(tn_finetune *f, float **w, float **g, float **mom, long *n);
