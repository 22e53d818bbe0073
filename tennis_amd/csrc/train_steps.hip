// C ABI of libtennis_hip.so (see include/tennis_hip.h): the temporal head's training step (tn_head_*) and the two frame-trained steps
// on the fine-tuning step's backbone, the CNN-RNN step (tn_cnnrnn_trainer_*: the head on top) and the frame-mode captioner step
// (tn_gnmt_frames_trainer_*: the captioner's trainer on top).  What those two share is FrameBackbone.
#include <string>
#include <vector>

#include "api_internal.h"
#include "linear.h"
#include "rnn.h"
#include "train.h"

// ---- temporal-head training step -----------------------------------------------------
struct tn_head : TrainParams, HeadOffsets {
  int F, H, C, maxB, maxT;
  int G;                           // gates per cell: 3 GRU, 4 LSTM
  float *mom;                      // [n] momentum, next to the parameters w and the gradients g
  float *whT;                      // [2][H][G*H] transposed h2h for the forward recurrence
  float *gi, *seq, *gates, *pooled, *dlog, *dpool, *dseq, *dgi, *dgh, *hprev, *logits, *loss;
  int32_t *arg;
  const float *feats = nullptr;    // tn_head_set_features: the caller's (feat_rows, F) table of row stride feat_ld, borrowed
  int feat_rows = 0, feat_ld = 0;
};

static int head_refresh_whT(tn_head *h) {
  for (int d = 0; d < 2; ++d)
    TN_TRY(launch_transpose_f32(h->w + h->o_wh + (long)d * h->G * h->H * h->H, h->G * h->H, h->H,
                                h->whT + (long)d * h->H * h->G * h->H, h->ctx->stream));
  return TN_OK;
}

extern "C" int tn_head_create(tn_ctx *ctx, tn_rnn_kind kind, int input_size, int hidden, int classes, const tn_param *params,
                              int n_params, const char *rnn_prefix, const char *dense_prefix, int max_batch,
                              int max_steps, tn_head **out) {
  TN_REQUIRE(ctx && params && rnn_prefix && dense_prefix && out, "tn_head_create: null argument");
  TN_REQUIRE(kind == TN_RNN_GRU || kind == TN_RNN_LSTM, "tn_head_create: type must be 'gru' or 'lstm'");
  const int G = kind == TN_RNN_GRU ? 3 : 4;
  TN_REQUIRE(input_size > 0 && hidden > 0 && hidden % 4 == 0 && G * hidden <= 2048 && classes > 0 && max_batch > 0 &&
                 max_steps > 0, "tn_head_create: bad shape (gates*hidden must be <= 2048, hidden % 4 == 0)");
  TN_ON_DEVICE(ctx->device);
  const int F = input_size, H = hidden, C = classes, GH = G * hidden;
  tn_head *h = new tn_head();
  h->ctx = ctx; h->G = G; h->F = F; h->H = H; h->C = C; h->maxB = max_batch; h->maxT = max_steps;
  h->table = head_param_table(G, F, H, C, rnn_prefix, dense_prefix, h);
  h->n = h->table.n;
  auto fail = [&](int rc) { h->pool.release(); delete h; return rc; };
  std::vector<float> w, st;
  if (!h->table.load(ParamMap(params, n_params), w, st)) return fail(TN_ERR_MISSING);
  h->w = h->pool.upload(w);
  const size_t rows = (size_t)max_batch * max_steps;
  auto fl = [&](size_t n) { return h->pool.alloc<float>(n); };
  h->g = fl(h->n); h->mom = fl(h->n); h->whT = fl(2L * H * GH);
  h->gi = fl(rows * 2 * GH); h->seq = fl(rows * 2 * H); h->gates = fl(2 * rows * (G + 1) * H);
  h->pooled = fl((size_t)max_batch * 2 * H); h->dlog = fl((size_t)max_batch * C); h->dpool = fl((size_t)max_batch * 2 * H);
  h->dseq = fl(rows * 2 * H); h->dgi = fl(rows * 2 * GH); h->dgh = fl(rows * 2 * GH); h->hprev = fl(2 * rows * H);
  h->logits = fl((size_t)max_batch * C); h->loss = fl(max_batch);
  h->arg = h->pool.alloc<int32_t>((size_t)max_batch * 2 * H);
  if (h->pool.failed) { tn_set_error("device allocation failed"); return fail(TN_ERR_NOMEM); }
  auto init = [&]() -> int {               // (a lambda: what fails in here leaves through `fail`, with the pool and the handle)
    TN_HIP_CHECK(hipMemsetAsync(h->mom, 0, h->n * sizeof(float), ctx->stream));
    TN_HIP_CHECK(hipMemsetAsync(h->g, 0, h->n * sizeof(float), ctx->stream));
    return head_refresh_whT(h);
  };
  if (const int rc = init()) return fail(rc);
  *out = h;
  return TN_OK;
}

// The head's step on x (B*T, F; rows b*T + t).  dx non-null: also the gradient with respect to x, dX = dGI W_ih (M, F; row
// stride ldx, assigned) - what the end-to-end CNN-RNN step hands to the backbone's backward.
// rows non-null: x is never materialised - row m of it is row rows[m] of the handle's feature table (tn_head_set_features),
// gathered inside the two kernels that read x (the i2h projection and dW_ih = dGI^T X).  labels null: the forward half only
// (through the logits; gradients, momentum and parameters untouched).
static int head_step(tn_head *h, const float *x, const int32_t *rows, const int32_t *labels, int B, int T, float *loss, float *logits,
                     float *dx, int ldx) {
  hipStream_t s = h->ctx->stream;
  const int F = h->F, H = h->H, C = h->C, GH = h->G * h->H, M = B * T;
  const bool lstm = h->G == 4;
  float *w = h->w, *g = h->g;
  // forward: one i2h GEMM for both directions, recurrence with saved gates, max over T (argmax kept), Dense
  if (rows) TN_TRY(launch_linear_f32_rows(h->feats, h->feat_ld, rows, h->feat_rows, w + h->o_wi, F, w + h->o_bi, h->gi, 2 * GH, M, 2 * GH, F, 0, s));
  else TN_TRY(launch_linear_f32(x, F, w + h->o_wi, F, w + h->o_bi, h->gi, 2 * GH, M, 2 * GH, F, 0, s));
  TN_TRY(launch_rnn_recurrent(h->G, h->gi, 2 * GH, h->whT, w + h->o_bh, nullptr, h->seq, 2 * H, nullptr, nullptr, B, T, H, 2, s,
                              h->gates));
  TN_TRY(launch_pool_max_arg(h->seq, B, T, 2 * H, h->pooled, h->arg, s));
  TN_TRY(launch_linear_f32(h->pooled, 2 * H, w + h->o_wd, 2 * H, w + h->o_bd, h->logits, C, B, C, 2 * H, 0, s));
  if (!labels) {
    if (logits) TN_HIP_CHECK(hipMemcpyAsync(logits, h->logits, sizeof(float) * B * C, hipMemcpyDeviceToDevice, s));
    return TN_OK;
  }
  TN_TRY(launch_softmax_ce(h->logits, labels, B, C, h->loss, h->dlog, s));
  // backward
  TN_TRY(launch_dense_bwd(h->dlog, h->pooled, w + h->o_wd, B, C, 2 * H, g + h->o_wd, g + h->o_bd, h->dpool, s));
  TN_TRY(launch_scatter_pool_grad(h->dpool, h->arg, B, T, 2 * H, h->dseq, s));
  TN_TRY(launch_rnn_bptt(h->G, h->seq, h->gates, h->dseq, w + h->o_wh, h->dgi, h->dgh, h->hprev, B, T, H, s));
  const float *dgh = lstm ? h->dgi : h->dgh;   // LSTM: one pre-activation gradient feeds both branches
  if (rows) TN_TRY(launch_gemm_tn_f32_rows(h->dgi, 2 * GH, h->feats, h->feat_ld, rows, h->feat_rows, g + h->o_wi, F, 2 * GH, F, M, s));
  else TN_TRY(launch_gemm_tn_f32(h->dgi, 2 * GH, x, F, g + h->o_wi, F, 2 * GH, F, M, s));      // dW_ih = dGI^T X
  TN_TRY(launch_colsum_f32(h->dgi, 2 * GH, M, 2 * GH, g + h->o_bi, s));
  for (int d = 0; d < 2; ++d)                                                              // dW_hh = dGH^T H_prev
    TN_TRY(launch_gemm_tn_f32(dgh + d * GH, 2 * GH, h->hprev + (long)d * M * H, H, g + h->o_wh + (long)d * GH * H, H,
                              GH, H, M, s));
  TN_TRY(launch_colsum_f32(dgh, 2 * GH, M, 2 * GH, g + h->o_bh, s));
  if (dx) TN_TRY(launch_gemm_nn_f32(h->dgi, 2 * GH, w + h->o_wi, F, dx, ldx, M, F, 2 * GH, 0, s));   // dX = dGI W_ih
  if (loss) TN_HIP_CHECK(hipMemcpyAsync(loss, h->loss, sizeof(float) * B, hipMemcpyDeviceToDevice, s));
  if (logits) TN_HIP_CHECK(hipMemcpyAsync(logits, h->logits, sizeof(float) * B * C, hipMemcpyDeviceToDevice, s));
  return TN_OK;
}

// the one bounds check of the three tn_head_forward_* entries; fn: the entry's name, for the message
static int head_check_shape(const char *fn, const tn_head *h, int B, int T) {
  TN_REQUIRE(B > 0 && B <= h->maxB && T > 0 && T <= h->maxT, std::string(fn) + ": batch / steps exceed the maxima");
  return TN_OK;
}

extern "C" int tn_head_forward_backward(tn_head *h, const float *x, const int32_t *labels, int B, int T, float *loss,
                                        float *logits) {
  TN_REQUIRE(h && x && labels, "tn_head_forward_backward: null argument");
  TN_TRY(head_check_shape("tn_head_forward_backward", h, B, T));
  TN_ON_DEVICE(h->ctx->device);
  return head_step(h, x, nullptr, labels, B, T, loss, logits, nullptr, 0);
}

extern "C" int tn_head_set_features(tn_head *h, const float *feats, int rows, int ld) {
  TN_REQUIRE(h && feats, "tn_head_set_features: null argument");
  TN_REQUIRE(rows > 0 && ld >= h->F, "tn_head_set_features: needs rows > 0 and ld >= the handle's input size");
  h->feats = feats; h->feat_rows = rows; h->feat_ld = ld;
  return TN_OK;
}

extern "C" int tn_head_forward_backward_rows(tn_head *h, const int32_t *row_idx, const int32_t *labels, int B, int T, float *loss,
                                             float *logits) {
  TN_REQUIRE(h && row_idx && labels, "tn_head_forward_backward_rows: null argument");
  TN_REQUIRE(h->feats, "tn_head_forward_backward_rows: no feature table (call tn_head_set_features first)");
  TN_TRY(head_check_shape("tn_head_forward_backward_rows", h, B, T));
  TN_ON_DEVICE(h->ctx->device);
  return head_step(h, nullptr, row_idx, labels, B, T, loss, logits, nullptr, 0);
}

extern "C" int tn_head_forward_rows(tn_head *h, const int32_t *row_idx, int B, int T, float *logits) {
  TN_REQUIRE(h && row_idx && logits, "tn_head_forward_rows: null argument");
  TN_REQUIRE(h->feats, "tn_head_forward_rows: no feature table (call tn_head_set_features first)");
  TN_TRY(head_check_shape("tn_head_forward_rows", h, B, T));
  TN_ON_DEVICE(h->ctx->device);
  return head_step(h, nullptr, row_idx, nullptr, B, T, nullptr, logits, nullptr, 0);
}

extern "C" int tn_head_buffers(tn_head *h, float **params_dev, float **grads_dev, int64_t *numel) {
  return train_buffers("tn_head_buffers", h, params_dev, grads_dev, numel);
}

// the update alone; scale non-null: the clipped form, on the scale of a reduction the caller has queued
static int head_sgd_update(tn_head *h, float lr, float momentum, float wd, float rescale_grad, const float *scale) {
  TN_TRY(launch_sgd_momentum(h->w, h->g, h->mom, h->n, lr, momentum, wd, rescale_grad, h->ctx->stream, scale));
  return head_refresh_whT(h);
}

extern "C" int tn_head_sgd_step(tn_head *h, float lr, float momentum, float wd, float rescale_grad) {
  TN_REQUIRE(h, "tn_head_sgd_step: null handle");
  TN_ON_DEVICE(h->ctx->device);
  if (!h->clip.on()) return head_sgd_update(h, lr, momentum, wd, rescale_grad, nullptr);
  TN_TRY(h->clip.reduce(h->ctx, h->g, h->n, nullptr, 0, rescale_grad));
  return head_sgd_update(h, lr, momentum, wd, rescale_grad, h->clip.scale());
}

extern "C" int tn_head_set_clip(tn_head *h, float max_norm) {
  TN_REQUIRE(h, "tn_head_set_clip: null handle");
  return h->clip.set("tn_head_set_clip", h->ctx, max_norm);
}
extern "C" int tn_head_clip_stats(tn_head *h, float *norm, float *scale, int64_t *clipped_steps) {
  TN_REQUIRE(h, "tn_head_clip_stats: null handle");
  return h->clip.stats("tn_head_clip_stats", h->ctx, norm, scale, clipped_steps);
}

extern "C" int tn_head_read_param(tn_head *h, const char *name, int gradient, float *out_host, int64_t capacity, int64_t *numel) {
  return train_read_param("tn_head_read_param", h, name, gradient, out_host, capacity, numel);
}

extern "C" int tn_head_destroy(tn_head *h) {
  if (!h) return TN_OK;
  TnDeviceGuard tn_dg_(h->ctx->device);
  (void)hipStreamSynchronize(h->ctx->stream);
  h->clip.release();
  h->pool.release();
  delete h;
  return TN_OK;
}

// ---- the backbone of the two frame-trained steps ---------------------------------------
// Both handles below are the fine-tuning step's backbone (finetune.hip, built without its classifier) over the frames of a step
// with a part of their own on its features, trained by one loss, one clipping norm and one update.  This is the backbone's half,
// held by value, and the one place that decides what a frozen backbone means (docs/numerics.md): its BatchNorms still normalise
// with the batch statistics and still move their running statistics; only its backward and its update are skipped, and its
// gradient is no part of the clipping norm.
struct FrameBackbone {
  tn_ctx *ctx = nullptr;
  tn_finetune *bb = nullptr;
  bool frozen = false;
  std::string prefix;           // of the backbone's parameter names
  int F = 0;                    // the feature width: what the part on top reads per frame
  GradClip clip;                // one norm over backbone + the part on top, one scale for both updates

  // fn: the entry's name, frames_are: what its `frames` count, in its own words - both for the message of a device too small
  int create(const char *fn, const char *frames_are, tn_ctx *c, const tn_param *params, int n_params, const char *backbone_prefix,
             int height, int width, int frames, int freeze) {
    long fit = -1;
    const int rc = ft_create(c, params, n_params, backbone_prefix, nullptr, height, width, 0, frames, &bb, &fit);
    if (rc == TN_ERR_NOMEM && fit >= 0)
      tn_set_error(std::string(fn) + ": " + std::to_string(frames) + " frames (" + frames_are + ") of " + std::to_string(height) + "x" +
                   std::to_string(width) + " do not fit the device; about " + std::to_string(fit) + " would");
    if (rc) return rc;
    ctx = c; frozen = freeze != 0; prefix = backbone_prefix; F = ft_feature_dim(bb);
    return TN_OK;
  }
  // backbone forward of x (n frames; training-mode BatchNorm over all of them) -> head(features, d loss / d features or null when
  // frozen, F): the step of the part on top -> backbone backward unless frozen -> the running statistics, either way
  template <typename Head>
  int step(const float *x, int n, Head head) {
    TN_TRY(ft_forward_features(bb, x, n));
    TN_TRY(head(ft_features(bb), frozen ? nullptr : ft_feature_grad(bb), F));
    if (!frozen) TN_TRY(ft_backward_features(bb, n));
    ft_update_running(bb);
    TN_HIP_CHECK(hipGetLastError());
    return TN_OK;
  }
  // *scale: null with clipping off; else the scale of the reduction this queues over (the backbone's gradient unless frozen, the
  // gradient head_g of the part on top) - what both updates of the step take
  int clip_scale(const float *head_g, long head_n, float rescale, const float **scale) {
    *scale = nullptr;
    if (!clip.on()) return TN_OK;
    float *g = nullptr;
    int64_t n = 0;
    if (!frozen) TN_TRY(tn_finetune_buffers(bb, nullptr, &g, &n));
    TN_TRY(clip.reduce(ctx, g, n, head_g, head_n, rescale));
    *scale = clip.scale();
    return TN_OK;
  }
  bool updates() const { return !frozen; }                  // frozen: the backbone's parameters are not touched (grad_req 'null')
  bool owns(const std::string &name) const { return name.rfind(prefix, 0) == 0; }
  void destroy() {                                          // after the part on top; (each drains the one stream)
    tn_finetune_destroy(bb);
    TnDeviceGuard tn_dg_(ctx->device);
    clip.release();
  }
};

// ---- end-to-end CNN-RNN training step -------------------------------------------------
// reference train.py:197-236 (--window > 1 --temp_pool gru|lstm, no --feats_model): the backbone over the batch*steps frames
// (features in rows b*steps + t), the temporal head above on its features, dX straight into the backbone's feature gradient.
struct tn_cnnrnn_trainer {
  FrameBackbone bb;
  tn_head *head;
  int B, T, H, W;
  std::string rnn_prefix, dense_prefix;
};

extern "C" int tn_cnnrnn_trainer_create(tn_ctx *ctx, tn_rnn_kind kind, const tn_param *params, int n_params,
                                        const char *backbone_prefix, const char *rnn_prefix, const char *dense_prefix, int height,
                                        int width, int classes, int batch, int steps, int freeze_backbone,
                                        tn_cnnrnn_trainer **out) {
  TN_REQUIRE(ctx && params && backbone_prefix && rnn_prefix && dense_prefix && out, "tn_cnnrnn_trainer_create: null argument");
  TN_REQUIRE(kind == TN_RNN_GRU || kind == TN_RNN_LSTM, "tn_cnnrnn_trainer_create: type must be 'gru' or 'lstm'");
  TN_REQUIRE(height > 0 && width > 0 && height % 32 == 0 && height == width,
             "tn_cnnrnn_trainer_create: frames must be square with a side divisible by 32");
  TN_REQUIRE(classes > 0, "tn_cnnrnn_trainer_create: classes must be positive");
  TN_REQUIRE(batch > 0 && steps > 0 && (long)batch * steps <= (1L << 20), "tn_cnnrnn_trainer_create: bad batch / steps");
  TN_ON_DEVICE(ctx->device);
  // the hidden size: <rnn_prefix>l0_i2h_bias has gates * hidden entries
  const int G = kind == TN_RNN_GRU ? 3 : 4;
  const std::string bias_name = std::string(rnn_prefix) + "l0_i2h_bias";
  const int hidden = (int)(ParamMap(params, n_params).numel(bias_name) / G);
  if (hidden <= 0) { tn_set_error("missing parameter: " + bias_name); return TN_ERR_MISSING; }
  FrameBackbone bb;
  TN_TRY(bb.create("tn_cnnrnn_trainer_create", "batch x steps", ctx, params, n_params, backbone_prefix, height, width, batch * steps, freeze_backbone));
  tn_head *head = nullptr;
  const int rc = tn_head_create(ctx, kind, bb.F, hidden, classes, params, n_params, rnn_prefix, dense_prefix, batch, steps, &head);
  if (rc) { bb.destroy(); return rc; }
  *out = new tn_cnnrnn_trainer{bb, head, batch, steps, height, width, rnn_prefix, dense_prefix};
  return TN_OK;
}

extern "C" int tn_cnnrnn_trainer_forward_backward(tn_cnnrnn_trainer *t, const float *x, const int32_t *labels, int batch, int steps,
                                                  int height, int width, float *loss, float *logits) {
  TN_REQUIRE(t && x && labels, "tn_cnnrnn_trainer_forward_backward: null argument");
  TN_REQUIRE(batch == t->B && steps == t->T,
             "tn_cnnrnn_trainer_forward_backward: batch and steps must equal the handle's (batch x steps frames, BatchNorm statistics over all)");
  TN_REQUIRE(height == t->H && width == t->W, "tn_cnnrnn_trainer_forward_backward: the frame size must equal the handle's");
  TN_ON_DEVICE(t->bb.ctx->device);
  return t->bb.step(x, t->B * t->T, [&](const float *feat, float *dfeat, int F) {
    return head_step(t->head, feat, nullptr, labels, t->B, t->T, loss, logits, dfeat, F);
  });
}

extern "C" int tn_cnnrnn_trainer_buffers(tn_cnnrnn_trainer *t, float **backbone_params, float **backbone_grads, int64_t *backbone_numel,
                                         float **head_params, float **head_grads, int64_t *head_numel) {
  TN_REQUIRE(t, "tn_cnnrnn_trainer_buffers: null handle");
  TN_TRY(tn_finetune_buffers(t->bb.bb, backbone_params, backbone_grads, backbone_numel));
  return tn_head_buffers(t->head, head_params, head_grads, head_numel);
}

extern "C" int tn_cnnrnn_trainer_sgd_step(tn_cnnrnn_trainer *t, float lr, float momentum, float wd, float rescale_grad) {
  TN_REQUIRE(t, "tn_cnnrnn_trainer_sgd_step: null handle");
  TN_ON_DEVICE(t->bb.ctx->device);
  const float *scale = nullptr;
  TN_TRY(t->bb.clip_scale(t->head->g, t->head->n, rescale_grad, &scale));
  if (t->bb.updates()) TN_TRY(ft_sgd_update(t->bb.bb, lr, momentum, wd, rescale_grad, scale));
  return head_sgd_update(t->head, lr, momentum, wd, rescale_grad, scale);
}

extern "C" int tn_cnnrnn_trainer_set_clip(tn_cnnrnn_trainer *t, float max_norm) {
  TN_REQUIRE(t, "tn_cnnrnn_trainer_set_clip: null handle");
  return t->bb.clip.set("tn_cnnrnn_trainer_set_clip", t->bb.ctx, max_norm);
}
extern "C" int tn_cnnrnn_trainer_clip_stats(tn_cnnrnn_trainer *t, float *norm, float *scale, int64_t *clipped_steps) {
  TN_REQUIRE(t, "tn_cnnrnn_trainer_clip_stats: null handle");
  return t->bb.clip.stats("tn_cnnrnn_trainer_clip_stats", t->bb.ctx, norm, scale, clipped_steps);
}

extern "C" int tn_cnnrnn_trainer_read_param(tn_cnnrnn_trainer *t, const char *name, int gradient, float *out_host, int64_t capacity,
                                            int64_t *numel) {
  TN_REQUIRE(t && name && out_host && numel, "tn_cnnrnn_trainer_read_param: null argument");
  const std::string n(name);
  if (n.rfind(t->rnn_prefix, 0) == 0 || n.rfind(t->dense_prefix, 0) == 0)
    return tn_head_read_param(t->head, name, gradient, out_host, capacity, numel);
  TN_REQUIRE(t->bb.owns(n), "tn_cnnrnn_trainer_read_param: unknown parameter name");
  return tn_finetune_read_param(t->bb.bb, name, gradient, out_host, capacity, numel);
}

extern "C" int tn_cnnrnn_trainer_set_matmul(tn_cnnrnn_trainer *t, int mode) {
  TN_REQUIRE(t, "tn_cnnrnn_trainer_set_matmul: null handle");
  return tn_finetune_set_matmul(t->bb.bb, mode);
}
extern "C" int tn_cnnrnn_trainer_matmul_stats(tn_cnnrnn_trainer *t, int64_t *f32_launches, int64_t *fp32x3_launches) {
  TN_REQUIRE(t, "tn_cnnrnn_trainer_matmul_stats: null handle");
  return tn_finetune_matmul_stats(t->bb.bb, f32_launches, fp32x3_launches);
}

extern "C" int tn_cnnrnn_trainer_destroy(tn_cnnrnn_trainer *t) {
  if (!t) return TN_OK;
  tn_head_destroy(t->head);
  t->bb.destroy();
  delete t;
  return TN_OK;
}

// ---- end-to-end frame-mode captioner training step ------------------------------------
// reference train_gnmt.py:148-203 without --feats_model: src_embed = TimeDistributed(FrameModel(DenseNet121.features).backbone)
// inside the NMTModel, trained (or frozen, :164-166) by the same loss.backward() / trainer.step(1) (:334-337).  The backbone over
// the batch * steps frames of the padded clips, the captioner's step (captioner_train.hip) on its features.
struct tn_gnmt_frames_trainer {
  FrameBackbone bb;
  tn_gnmt_trainer *cap;
  int side, maxB, maxT, maxN;
  long step;                    // Adam's update count, one for both parts
  std::string prefix;
};

extern "C" int tn_gnmt_frames_trainer_create(tn_ctx *ctx, const tn_param *params, int n_params, const char *backbone_prefix,
                                             const char *prefix, tn_rnn_kind cell_kind, int hidden, int embed, int vocab, int num_layers,
                                             int num_bi_layers, int flags, int side, int max_batch, int max_src_len, int max_tgt_len,
                                             int max_frames, int freeze_backbone, tn_gnmt_frames_trainer **out) {
  TN_REQUIRE(ctx && params && backbone_prefix && prefix && out, "tn_gnmt_frames_trainer_create: null argument");
  TN_REQUIRE(side > 0 && side % 32 == 0, "tn_gnmt_frames_trainer_create: frames must be square with a side divisible by 32");
  TN_REQUIRE(max_batch > 0 && max_src_len > 0 && max_frames > 0 && max_frames <= 65535,
             "tn_gnmt_frames_trainer_create: bad max_batch / max_src_len / max_frames");
  TN_ON_DEVICE(ctx->device);
  FrameBackbone bb;
  TN_TRY(bb.create("tn_gnmt_frames_trainer_create", "the longest padded batch, batch x steps", ctx, params, n_params, backbone_prefix, side,
                   side, max_frames, freeze_backbone));
  const int F = bb.F, G = cell_kind == TN_RNN_GRU ? 3 : 4;
  // the captioner's first layer reads the backbone's features: refuse parameters made for another width
  const std::string w0 = std::string(prefix) + (num_bi_layers > 0 ? "enc_rnn0_l_i2h_weight" : "enc_rnn0_i2h_weight");
  const int64_t w0_numel = ParamMap(params, n_params).numel(w0);
  if (w0_numel >= 0 && w0_numel != (int64_t)G * hidden * F) {
    tn_set_error("tn_gnmt_frames_trainer_create: " + w0 + " is not (gates * hidden, " + std::to_string(F) + "), the backbone's feature width");
    bb.destroy();
    return TN_ERR_INVALID;
  }
  tn_gnmt_trainer *cap = nullptr;
  int rc = tn_gnmt_trainer_create_ex(ctx, params, n_params, prefix, cell_kind, F, hidden, embed, vocab, num_layers, num_bi_layers, flags,
                                     max_batch, max_src_len, max_tgt_len, &cap);
  if (!rc && !freeze_backbone) rc = ft_enable_adam(bb.bb);
  if (rc) { tn_gnmt_trainer_destroy(cap); bb.destroy(); return rc; }
  *out = new tn_gnmt_frames_trainer{bb, cap, side, max_batch, max_src_len, max_frames, 0, prefix};
  return TN_OK;
}

// frames into the backbone's staging buffer, zeros in the padded slots (they go through the backbone with the others, as TimeDistributed sends
// them, and count in its batch statistics) -> its features, rows b * steps + t = the captioner's (batch, steps, F) source as it stands
extern "C" int tn_gnmt_frames_trainer_forward_backward(tn_gnmt_frames_trainer *t, const float *frames, const int32_t *src_valid_len,
                                                       const int32_t *tgt, int ld, const int32_t *tgt_valid_len, int batch, int steps,
                                                       int tgt_len, float *loss, float *logits_out) {
  TN_REQUIRE(t && frames && src_valid_len && tgt && tgt_valid_len && loss, "tn_gnmt_frames_trainer_forward_backward: null argument");
  TN_REQUIRE(batch > 0 && batch <= t->maxB, "tn_gnmt_frames_trainer_forward_backward: batch exceeds max_batch");
  TN_REQUIRE(steps > 0 && steps <= t->maxT, "tn_gnmt_frames_trainer_forward_backward: steps exceed max_src_len");
  TN_REQUIRE((long)batch * steps <= t->maxN, "tn_gnmt_frames_trainer_forward_backward: batch * steps exceeds max_frames");
  TN_REQUIRE(tgt_len >= 2 && ld >= tgt_len, "tn_gnmt_frames_trainer_forward_backward: need tgt_len >= 2 and ld >= tgt_len");
  TN_ON_DEVICE(t->bb.ctx->device);
  float *x = ft_frame_staging(t->bb.bb);
  TN_TRY(launch_stage_frames(frames, src_valid_len, batch, steps, (long)t->side * t->side * 3, x, t->bb.ctx->stream));
  return t->bb.step(x, batch * steps, [&](const float *feat, float *dfeat, int F) {
    return gnmt_trainer_step(t->cap, feat, src_valid_len, tgt, ld, tgt_valid_len, batch, steps, tgt_len, loss, logits_out, dfeat, F);
  });
}

extern "C" int tn_gnmt_frames_trainer_buffers(tn_gnmt_frames_trainer *t, float **backbone_params, float **backbone_grads,
                                              int64_t *backbone_numel, float **params_dev, float **grads_dev, int64_t *numel) {
  TN_REQUIRE(t, "tn_gnmt_frames_trainer_buffers: null handle");
  TN_TRY(tn_finetune_buffers(t->bb.bb, backbone_params, backbone_grads, backbone_numel));
  return tn_gnmt_trainer_buffers(t->cap, params_dev, grads_dev, numel);
}

extern "C" int tn_gnmt_frames_trainer_set_dropout(tn_gnmt_frames_trainer *t, float p, uint64_t seed) {
  TN_REQUIRE(t, "tn_gnmt_frames_trainer_set_dropout: null handle");
  return tn_gnmt_trainer_set_dropout(t->cap, p, seed);
}

// gluon.Trainer(model.collect_params(), 'adam').step(1) (train_gnmt.py:310,337) over both parts with one update count
extern "C" int tn_gnmt_frames_trainer_adam_step(tn_gnmt_frames_trainer *t, float lr, float beta1, float beta2, float epsilon) {
  TN_REQUIRE(t, "tn_gnmt_frames_trainer_adam_step: null handle");
  TN_ON_DEVICE(t->bb.ctx->device);
  float *cg = nullptr;
  int64_t cn = 0;
  TN_TRY(tn_gnmt_trainer_buffers(t->cap, nullptr, &cg, &cn));
  const float *scale = nullptr;
  TN_TRY(t->bb.clip_scale(cg, cn, 1.f, &scale));
  t->step += 1;
  if (t->bb.updates()) TN_TRY(ft_adam_step(t->bb.bb, lr, beta1, beta2, epsilon, t->step, scale));
  return gnmt_trainer_adam(t->cap, lr, beta1, beta2, epsilon, t->step, scale);
}

extern "C" int tn_gnmt_frames_trainer_set_clip(tn_gnmt_frames_trainer *t, float max_norm) {
  TN_REQUIRE(t, "tn_gnmt_frames_trainer_set_clip: null handle");
  return t->bb.clip.set("tn_gnmt_frames_trainer_set_clip", t->bb.ctx, max_norm);
}
extern "C" int tn_gnmt_frames_trainer_clip_stats(tn_gnmt_frames_trainer *t, float *norm, float *scale, int64_t *clipped_steps) {
  TN_REQUIRE(t, "tn_gnmt_frames_trainer_clip_stats: null handle");
  return t->bb.clip.stats("tn_gnmt_frames_trainer_clip_stats", t->bb.ctx, norm, scale, clipped_steps);
}

extern "C" int tn_gnmt_frames_trainer_read_param(tn_gnmt_frames_trainer *t, const char *name, int gradient, float *out_host,
                                                 int64_t capacity, int64_t *numel) {
  TN_REQUIRE(t && name && out_host && numel, "tn_gnmt_frames_trainer_read_param: null argument");
  const std::string n(name);
  if (t->bb.owns(n)) return tn_finetune_read_param(t->bb.bb, name, gradient, out_host, capacity, numel);
  TN_REQUIRE(n.rfind(t->prefix, 0) == 0, "tn_gnmt_frames_trainer_read_param: unknown parameter name");
  return tn_gnmt_trainer_read_param(t->cap, name, gradient, out_host, capacity, numel);
}

extern "C" int tn_gnmt_frames_trainer_set_matmul(tn_gnmt_frames_trainer *t, int mode) {
  TN_REQUIRE(t, "tn_gnmt_frames_trainer_set_matmul: null handle");
  return tn_finetune_set_matmul(t->bb.bb, mode);
}
extern "C" int tn_gnmt_frames_trainer_matmul_stats(tn_gnmt_frames_trainer *t, int64_t *f32_launches, int64_t *fp32x3_launches) {
  TN_REQUIRE(t, "tn_gnmt_frames_trainer_matmul_stats: null handle");
  return tn_finetune_matmul_stats(t->bb.bb, f32_launches, fp32x3_launches);
}

extern "C" int tn_gnmt_frames_trainer_destroy(tn_gnmt_frames_trainer *t) {
  if (!t) return TN_OK;
  tn_gnmt_trainer_destroy(t->cap);
  t->bb.destroy();
  delete t;
  return TN_OK;
}
