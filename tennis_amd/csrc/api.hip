// C ABI of libtennis_hip.so (see include/tennis_hip.h): error string, context, Dense, bi-RNN, the dense windowed evaluation of the
// temporal heads, temporal pooling and the PRF1 histogram.  The DenseNet-121 frame encoder is encoder.hip; the temporal head's
// trainer and the two frame-trained steps are train_steps.hip.
#include <cstring>
#include <string>
#include <vector>

#include "api_internal.h"
#include "linear.h"
#include "rnn.h"
#include "rnn_window.h"
#include "step_maps.h"
#include "train.h"

// ---------------------------------------------------------------------------
static thread_local std::string g_err;
void tn_set_error(const std::string &msg) { g_err = msg; }
extern "C" const char *tn_last_error(void) { return g_err.c_str(); }
extern "C" int tn_version(void) { return 100; }

// ---- context ----------------------------------------------------------------
extern "C" int tn_ctx_create(int device, void *stream, int own_stream, tn_ctx **out) {
  TN_REQUIRE(out != nullptr, "tn_ctx_create: out is null");
  int n = 0;
  TN_HIP_CHECK(hipGetDeviceCount(&n));
  TN_REQUIRE(device >= 0 && device < n, "tn_ctx_create: no such device");
  TN_ON_DEVICE(device);
  tn_ctx *c = new tn_ctx();
  c->device = device;
  c->own_stream = own_stream != 0;
  if (c->own_stream) {
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete c;
      tn_set_error(std::string("hipStreamCreate: ") + hipGetErrorString(e));
      return TN_ERR_HIP;
    }
  } else {
    c->stream = (hipStream_t)stream;
  }
  *out = c;
  return TN_OK;
}
extern "C" void *tn_ctx_stream(tn_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }
extern "C" int tn_ctx_sync(tn_ctx *ctx) {
  TN_REQUIRE(ctx, "tn_ctx_sync: null ctx");
  TN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return TN_OK;
}
extern "C" int tn_ctx_destroy(tn_ctx *ctx) {
  if (!ctx) return TN_OK;
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return TN_OK;
}

// ---- Dense (struct tn_dense: api_internal.h) --------------------------------------

extern "C" int tn_dense_create(tn_ctx *ctx, const float *weight_host, const float *bias_host, int units,
                               int in_units, tn_dense **out) {
  TN_REQUIRE(ctx && weight_host && out, "tn_dense_create: null argument");
  TN_REQUIRE(units > 0 && in_units > 0, "tn_dense_create: bad shape");
  TN_ON_DEVICE(ctx->device);
  tn_dense *d = new tn_dense();
  d->ctx = ctx; d->units = units; d->in_units = in_units;
  d->w = d->pool.upload(std::vector<float>(weight_host, weight_host + (size_t)units * in_units));
  d->b = bias_host ? d->pool.upload(std::vector<float>(bias_host, bias_host + units)) : nullptr;
  if (d->pool.failed) { d->pool.release(); delete d; tn_set_error("device allocation failed"); return TN_ERR_NOMEM; }
  *out = d;
  return TN_OK;
}
extern "C" int tn_dense_forward(tn_dense *d, const float *x, int rows, float *y) {
  TN_REQUIRE(d && x && y, "tn_dense_forward: null argument");
  TN_REQUIRE(rows >= 0, "tn_dense_forward: negative rows");
  TN_ON_DEVICE(d->ctx->device);
  return launch_linear_f32(x, d->in_units, d->w, d->in_units, d->b, y, d->units, rows, d->units, d->in_units, 0,
                           d->ctx->stream);
}
extern "C" int tn_dense_step_maps(tn_dense *d, const float *pooled, const int32_t *steps, int batch, int window, float *tam) {
  TN_REQUIRE(d && pooled && steps && tam, "tn_dense_step_maps: null argument");
  TN_REQUIRE(batch > 0 && window >= 1, "tn_dense_step_maps: batch must be > 0 and window >= 1");
  TN_ON_DEVICE(d->ctx->device);
  return launch_step_maps(pooled, steps, d->w, batch, d->in_units, d->units, window, tam, d->ctx->stream);
}
extern "C" int tn_dense_destroy(tn_dense *d) {
  if (!d) return TN_OK;
  TnDeviceGuard tn_dg_(d->ctx->device);
  d->pool.release();
  delete d;
  return TN_OK;
}

// ---- bi-RNN ----------------------------------------------------------------------
struct tn_birnn {
  tn_ctx *ctx;
  DevPool pool;
  int gates, F, H, dirs, max_rows;
  float *wi;   // [dirs*G*H][F]   both directions stacked -> one i2h GEMM
  float *bi;   // [dirs*G*H]
  float *whT;  // [dirs][H][G*H]
  float *bh;   // [dirs][G*H]
  float *gi;   // workspace [max_rows][dirs*G*H]
};

extern "C" int tn_birnn_create(tn_ctx *ctx, tn_rnn_kind kind, int input_size, int hidden, const tn_param *params,
                               int n_params, const char *prefix_c, int bidirectional, int max_rows, tn_birnn **out) {
  TN_REQUIRE(ctx && params && prefix_c && out, "tn_birnn_create: null argument");
  TN_REQUIRE(kind == TN_RNN_GRU || kind == TN_RNN_LSTM, "tn_birnn_create: unknown cell kind");
  TN_REQUIRE(input_size > 0 && hidden > 0 && hidden % 4 == 0 && max_rows > 0, "tn_birnn_create: bad shape");
  const int G = kind == TN_RNN_GRU ? 3 : 4;
  TN_REQUIRE(G * hidden <= 2048, "tn_birnn_create: gates*hidden must be <= 2048");
  TN_ON_DEVICE(ctx->device);
  const std::string pre(prefix_c);
  ParamMap pm(params, n_params);
  const int dirs = bidirectional ? 2 : 1, GH = G * hidden;
  std::vector<float> wi((size_t)dirs * GH * input_size), bi((size_t)dirs * GH), whT((size_t)dirs * hidden * GH),
      bh((size_t)dirs * GH);
  for (int d = 0; d < dirs; ++d) {
    const std::string dp = pre + (d == 0 ? "l0_" : "r0_");
    const float *a = pm.get(dp + "i2h_weight", (int64_t)GH * input_size);
    const float *b = pm.get(dp + "h2h_weight", (int64_t)GH * hidden);
    const float *c = pm.get(dp + "i2h_bias", GH);
    const float *e = pm.get(dp + "h2h_bias", GH);
    if (!a || !b || !c || !e) return TN_ERR_MISSING;
    memcpy(&wi[(size_t)d * GH * input_size], a, sizeof(float) * GH * input_size);
    memcpy(&bi[(size_t)d * GH], c, sizeof(float) * GH);
    memcpy(&bh[(size_t)d * GH], e, sizeof(float) * GH);
    for (int j = 0; j < GH; ++j)
      for (int k = 0; k < hidden; ++k) whT[((size_t)d * hidden + k) * GH + j] = b[(size_t)j * hidden + k];
  }
  tn_birnn *r = new tn_birnn();
  r->ctx = ctx; r->gates = G; r->F = input_size; r->H = hidden; r->dirs = dirs; r->max_rows = max_rows;
  r->wi = r->pool.upload(wi); r->bi = r->pool.upload(bi); r->whT = r->pool.upload(whT); r->bh = r->pool.upload(bh);
  r->gi = (float *)r->pool.alloc((size_t)max_rows * dirs * GH * sizeof(float));
  if (r->pool.failed) {
    r->pool.release(); delete r; tn_set_error("device allocation failed"); return TN_ERR_NOMEM;
  }
  *out = r;
  return TN_OK;
}

extern "C" int tn_birnn_forward(tn_birnn *r, const float *x, int batch, int steps, const int32_t *valid_len,
                                float *seq, float *h_last, float *c_last) {
  TN_REQUIRE(r && x && seq, "tn_birnn_forward: null argument");
  TN_REQUIRE(batch > 0 && steps > 0 && (long)batch * steps <= r->max_rows, "tn_birnn_forward: B*T exceeds max_rows");
  TN_ON_DEVICE(r->ctx->device);
  hipStream_t s = r->ctx->stream;
  const int GH = r->gates * r->H, N = r->dirs * GH, rows = batch * steps;
  int rc = launch_linear_f32(x, r->F, r->wi, r->F, r->bi, r->gi, N, rows, N, r->F, 0, s);
  if (rc) return rc;
  if (valid_len) TN_HIP_CHECK(hipMemsetAsync(seq, 0, (size_t)rows * r->dirs * r->H * sizeof(float), s));
  return launch_rnn_recurrent(r->gates, r->gi, N, r->whT, r->bh, valid_len, seq, r->dirs * r->H, h_last, c_last,
                              batch, steps, r->H, r->dirs, s);
}
// tn_birnn_forward with x never materialised: row b * steps + t of x is row row_idx[b * steps + t] of table (n_rows, F; row stride
// ld), zeros where the index is negative; the i2h product gathers the rows while it stages them (api_internal.h).
int birnn_forward_rows(tn_birnn *r, const float *table, int n_rows, int ld, const int32_t *row_idx, int batch, int steps,
                       const int32_t *valid_len, float *seq, float *h_last, float *c_last) {
  TN_REQUIRE(r && table && row_idx && seq, "birnn_forward_rows: null argument");
  TN_REQUIRE(n_rows >= 1 && ld >= r->F, "birnn_forward_rows: needs n_rows >= 1 and ld >= input_size");
  TN_REQUIRE(batch > 0 && steps > 0 && (long)batch * steps <= r->max_rows, "birnn_forward_rows: B*T exceeds max_rows");
  TN_ON_DEVICE(r->ctx->device);
  hipStream_t s = r->ctx->stream;
  const int GH = r->gates * r->H, N = r->dirs * GH, rows = batch * steps;
  int rc = launch_linear_f32_padrows(table, ld, row_idx, n_rows, r->wi, r->F, r->bi, r->gi, N, rows, N, r->F, 0, s);
  if (rc) return rc;
  if (valid_len) TN_HIP_CHECK(hipMemsetAsync(seq, 0, (size_t)rows * r->dirs * r->H * sizeof(float), s));
  return launch_rnn_recurrent(r->gates, r->gi, N, r->whT, r->bh, valid_len, seq, r->dirs * r->H, h_last, c_last,
                              batch, steps, r->H, r->dirs, s);
}
extern "C" int tn_birnn_destroy(tn_birnn *r) {
  if (!r) return TN_OK;
  TnDeviceGuard tn_dg_(r->ctx->device);
  r->pool.release();
  delete r;
  return TN_OK;
}

// ---- dense windowed evaluation of the temporal heads ----------------------------------
struct tn_window_head {
  tn_ctx *ctx;
  DevPool pool;
  int gates, F, H, C, max_rows, max_samples;
  int rows;    // rows of the matrix the last project() saw; 0: none yet
  int nb;      // samples per workgroup of the recurrent kernel; 0: the library's choice
  float *wi;   // [2*G*H][F]   both directions stacked -> one i2h GEMM
  float *bi;   // [2*G*H]
  float *whT;  // [2][H][G*H]
  float *bh;   // [2][G*H]
  float *wd;   // [C][2H]
  float *bd;   // [C]
  float *gi;      // [max_rows][2*G*H]: the projection of every row of the matrix
  float *pooled;  // [max_samples][2H]
  int32_t *steps = nullptr;   // [max_samples][2H], allocated by the first *_tam call that brings no buffer of its own
};

extern "C" int tn_window_head_create(tn_ctx *ctx, tn_rnn_kind kind, int input_size, int hidden, int classes,
                                     const tn_param *params, int n_params, const char *rnn_prefix, const char *dense_prefix,
                                     int max_rows, int max_samples, tn_window_head **out) {
  TN_REQUIRE(ctx && params && rnn_prefix && dense_prefix && out, "tn_window_head_create: null argument");
  TN_REQUIRE(kind == TN_RNN_GRU || kind == TN_RNN_LSTM, "tn_window_head_create: unknown cell kind");
  const int G = kind == TN_RNN_GRU ? 3 : 4;
  TN_REQUIRE(input_size > 0 && hidden > 0 && hidden % 4 == 0 && G * hidden <= 1024 && classes > 0 && max_rows > 0 &&
                 max_samples > 0, "tn_window_head_create: bad shape (the windowed kernel serves gates*hidden <= 1024, hidden % 4 == 0; dense windowed "
                 "evaluation of a wider head is not supported)");
  TN_ON_DEVICE(ctx->device);
  ParamMap pm(params, n_params);
  const int F = input_size, H = hidden, C = classes, GH = G * hidden;
  std::vector<float> wi((size_t)2 * GH * F), bi((size_t)2 * GH), whT((size_t)2 * H * GH), bh((size_t)2 * GH);
  for (int d = 0; d < 2; ++d) {
    const std::string dp = std::string(rnn_prefix) + (d == 0 ? "l0_" : "r0_");
    const float *a = pm.get(dp + "i2h_weight", (int64_t)GH * F), *b = pm.get(dp + "h2h_weight", (int64_t)GH * H);
    const float *c = pm.get(dp + "i2h_bias", GH), *e = pm.get(dp + "h2h_bias", GH);
    if (!a || !b || !c || !e) return TN_ERR_MISSING;
    memcpy(&wi[(size_t)d * GH * F], a, sizeof(float) * GH * F);
    memcpy(&bi[(size_t)d * GH], c, sizeof(float) * GH);
    memcpy(&bh[(size_t)d * GH], e, sizeof(float) * GH);
    for (int j = 0; j < GH; ++j)
      for (int k = 0; k < H; ++k) whT[((size_t)d * H + k) * GH + j] = b[(size_t)j * H + k];
  }
  const float *wd = pm.get(std::string(dense_prefix) + "weight", (int64_t)C * 2 * H);
  const float *bd = pm.get(std::string(dense_prefix) + "bias", C);
  if (!wd || !bd) return TN_ERR_MISSING;
  tn_window_head *h = new tn_window_head();
  h->ctx = ctx; h->gates = G; h->F = F; h->H = H; h->C = C; h->max_rows = max_rows; h->max_samples = max_samples;
  h->rows = 0; h->nb = 0;
  h->wi = h->pool.upload(wi); h->bi = h->pool.upload(bi); h->whT = h->pool.upload(whT); h->bh = h->pool.upload(bh);
  h->wd = h->pool.upload(std::vector<float>(wd, wd + (size_t)C * 2 * H));
  h->bd = h->pool.upload(std::vector<float>(bd, bd + C));
  h->gi = (float *)h->pool.alloc((size_t)max_rows * 2 * GH * sizeof(float));
  h->pooled = (float *)h->pool.alloc((size_t)max_samples * 2 * H * sizeof(float));
  if (h->pool.failed) { h->pool.release(); delete h; tn_set_error("device allocation failed"); return TN_ERR_NOMEM; }
  *out = h;
  return TN_OK;
}

extern "C" int tn_window_head_project(tn_window_head *h, const float *feats, int rows) {
  TN_REQUIRE(h && feats, "tn_window_head_project: null argument");
  TN_REQUIRE(rows > 0 && rows <= h->max_rows, "tn_window_head_project: rows must be in [1, max_rows]");
  TN_ON_DEVICE(h->ctx->device);
  const int N = 2 * h->gates * h->H;
  h->rows = 0;
  const int rc = launch_linear_f32(feats, h->F, h->wi, h->F, h->bi, h->gi, N, rows, N, h->F, 0, h->ctx->stream);
  if (rc) return rc;
  h->rows = rows;
  return TN_OK;
}

extern "C" int tn_window_head_forward(tn_window_head *h, const int32_t *centre, const int32_t *lo, const int32_t *hi,
                                      int samples, int window, int stride, float *pooled, float *logits) {
  TN_REQUIRE(h && centre && lo && hi && logits, "tn_window_head_forward: null argument");
  TN_REQUIRE(h->rows > 0, "tn_window_head_forward: no projected matrix (call tn_window_head_project first)");
  TN_REQUIRE(samples > 0 && samples <= h->max_samples, "tn_window_head_forward: samples must be in [1, max_samples]");
  TN_REQUIRE(window >= 1 && stride >= 1, "tn_window_head_forward: window and stride must be >= 1");
  TN_ON_DEVICE(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  const int H = h->H;
  float *p = pooled ? pooled : h->pooled;
  const int rc = launch_rnn_window(h->gates, h->gi, 2 * h->gates * H, h->rows, h->whT, h->bh, centre, lo, hi, p, samples, window,
                                   stride, H, h->nb, s);
  if (rc) return rc;
  return launch_linear_f32(p, 2 * H, h->wd, 2 * H, h->bd, logits, h->C, samples, h->C, 2 * H, 0, s);
}

extern "C" int tn_window_head_forward_rows(tn_window_head *h, const int32_t *idx, int samples, int window, float *pooled,
                                           float *logits) {
  TN_REQUIRE(h && idx && logits, "tn_window_head_forward_rows: null argument");
  TN_REQUIRE(h->rows > 0, "tn_window_head_forward_rows: no projected matrix (call tn_window_head_project first)");
  TN_REQUIRE(samples > 0 && samples <= h->max_samples, "tn_window_head_forward_rows: samples must be in [1, max_samples]");
  TN_REQUIRE(window >= 1, "tn_window_head_forward_rows: window must be >= 1");
  TN_ON_DEVICE(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  const int H = h->H;
  float *p = pooled ? pooled : h->pooled;
  const int rc = launch_rnn_window_rows(h->gates, h->gi, 2 * h->gates * H, h->rows, h->whT, h->bh, idx, p, samples, window, H,
                                        h->nb, s);
  if (rc) return rc;
  return launch_linear_f32(p, 2 * H, h->wd, 2 * H, h->bd, logits, h->C, samples, h->C, 2 * H, 0, s);
}

// the steps buffer of a *_tam call: the caller's, or the handle's own (allocated at first use: a handle that never asks has none)
static int window_head_steps(tn_window_head *h, int32_t *steps, int32_t **out) {
  if (!steps && !h->steps) {
    h->steps = (int32_t *)h->pool.alloc((size_t)h->max_samples * 2 * h->H * sizeof(int32_t));
    if (!h->steps) { tn_set_error("device allocation failed"); return TN_ERR_NOMEM; }
  }
  *out = steps ? steps : h->steps;
  return TN_OK;
}

extern "C" int tn_window_head_forward_tam(tn_window_head *h, const int32_t *centre, const int32_t *lo, const int32_t *hi, int samples,
                                          int window, int stride, float *pooled, float *logits, int32_t *steps, float *tam) {
  TN_REQUIRE(h && centre && lo && hi && logits && tam, "tn_window_head_forward_tam: null argument");
  TN_REQUIRE(h->rows > 0, "tn_window_head_forward_tam: no projected matrix (call tn_window_head_project first)");
  TN_REQUIRE(samples > 0 && samples <= h->max_samples, "tn_window_head_forward_tam: samples must be in [1, max_samples]");
  TN_REQUIRE(window >= 1 && stride >= 1, "tn_window_head_forward_tam: window and stride must be >= 1");
  TN_ON_DEVICE(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  const int H = h->H;
  float *p = pooled ? pooled : h->pooled;
  int32_t *st = nullptr;
  int rc = window_head_steps(h, steps, &st);
  if (rc) return rc;
  rc = launch_rnn_window(h->gates, h->gi, 2 * h->gates * H, h->rows, h->whT, h->bh, centre, lo, hi, p, samples, window, stride, H,
                         h->nb, s, st);
  if (rc) return rc;
  rc = launch_linear_f32(p, 2 * H, h->wd, 2 * H, h->bd, logits, h->C, samples, h->C, 2 * H, 0, s);
  if (rc) return rc;
  return launch_step_maps(p, st, h->wd, samples, 2 * H, h->C, window, tam, s);
}

extern "C" int tn_window_head_forward_rows_tam(tn_window_head *h, const int32_t *idx, int samples, int window, float *pooled,
                                               float *logits, int32_t *steps, float *tam) {
  TN_REQUIRE(h && idx && logits && tam, "tn_window_head_forward_rows_tam: null argument");
  TN_REQUIRE(h->rows > 0, "tn_window_head_forward_rows_tam: no projected matrix (call tn_window_head_project first)");
  TN_REQUIRE(samples > 0 && samples <= h->max_samples, "tn_window_head_forward_rows_tam: samples must be in [1, max_samples]");
  TN_REQUIRE(window >= 1, "tn_window_head_forward_rows_tam: window must be >= 1");
  TN_ON_DEVICE(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  const int H = h->H;
  float *p = pooled ? pooled : h->pooled;
  int32_t *st = nullptr;
  int rc = window_head_steps(h, steps, &st);
  if (rc) return rc;
  rc = launch_rnn_window_rows(h->gates, h->gi, 2 * h->gates * H, h->rows, h->whT, h->bh, idx, p, samples, window, H, h->nb, s, st);
  if (rc) return rc;
  rc = launch_linear_f32(p, 2 * H, h->wd, 2 * H, h->bd, logits, h->C, samples, h->C, 2 * H, 0, s);
  if (rc) return rc;
  return launch_step_maps(p, st, h->wd, samples, 2 * H, h->C, window, tam, s);
}

extern "C" int tn_dbg_window_head_rows_per_group(tn_window_head *h, int nb) {
  TN_REQUIRE(h, "tn_dbg_window_head_rows_per_group: null argument");
  TN_REQUIRE(nb == 0 || nb == 4 || nb == 2 * h->gates, "tn_dbg_window_head_rows_per_group: 0 (default), 4 or twice the gates");
  h->nb = nb;
  return TN_OK;
}

extern "C" int tn_window_head_destroy(tn_window_head *h) {
  if (!h) return TN_OK;
  TnDeviceGuard tn_dg_(h->ctx->device);
  h->pool.release();
  delete h;
  return TN_OK;
}

extern "C" int tn_temporal_pool_windows(tn_ctx *ctx, const float *feats, int rows, int feat, const int32_t *centre,
                                        const int32_t *lo, const int32_t *hi, int samples, int window, int stride,
                                        tn_pool_kind kind, float *y) {
  TN_REQUIRE(ctx && feats && centre && lo && hi && y, "tn_temporal_pool_windows: null argument");
  TN_REQUIRE(rows > 0 && feat > 0 && samples > 0, "tn_temporal_pool_windows: bad shape");
  TN_REQUIRE(window >= 1 && stride >= 1, "tn_temporal_pool_windows: window and stride must be >= 1");
  TN_REQUIRE(kind == TN_POOL_MAX || kind == TN_POOL_MEAN, "tn_temporal_pool_windows: unknown pool kind");
  TN_ON_DEVICE(ctx->device);
  return launch_temporal_pool_windows(feats, rows, feat, centre, lo, hi, samples, window, stride, (int)kind, y, ctx->stream);
}

extern "C" int tn_temporal_pool_rows(tn_ctx *ctx, const float *feats, int rows, int feat, const int32_t *idx, int samples,
                                     int window, tn_pool_kind kind, float *y) {
  TN_REQUIRE(ctx && feats && idx && y, "tn_temporal_pool_rows: null argument");
  TN_REQUIRE(rows > 0 && feat > 0 && samples > 0, "tn_temporal_pool_rows: bad shape");
  TN_REQUIRE(window >= 1, "tn_temporal_pool_rows: window must be >= 1");
  TN_REQUIRE(kind == TN_POOL_MAX || kind == TN_POOL_MEAN, "tn_temporal_pool_rows: unknown pool kind");
  TN_ON_DEVICE(ctx->device);
  return launch_temporal_pool_rows(feats, rows, feat, idx, samples, window, (int)kind, y, ctx->stream);
}

extern "C" int tn_temporal_pool_windows_arg(tn_ctx *ctx, const float *feats, int rows, int feat, const int32_t *centre,
                                            const int32_t *lo, const int32_t *hi, int samples, int window, int stride, float *y,
                                            int32_t *arg) {
  TN_REQUIRE(ctx && feats && centre && lo && hi && y && arg, "tn_temporal_pool_windows_arg: null argument");
  TN_REQUIRE(rows > 0 && feat > 0 && samples > 0, "tn_temporal_pool_windows_arg: bad shape");
  TN_REQUIRE(window >= 1 && stride >= 1, "tn_temporal_pool_windows_arg: window and stride must be >= 1");
  TN_ON_DEVICE(ctx->device);
  return launch_temporal_pool_windows(feats, rows, feat, centre, lo, hi, samples, window, stride, (int)TN_POOL_MAX, y, ctx->stream,
                                      arg);
}

extern "C" int tn_temporal_pool_rows_arg(tn_ctx *ctx, const float *feats, int rows, int feat, const int32_t *idx, int samples,
                                         int window, float *y, int32_t *arg) {
  TN_REQUIRE(ctx && feats && idx && y && arg, "tn_temporal_pool_rows_arg: null argument");
  TN_REQUIRE(rows > 0 && feat > 0 && samples > 0, "tn_temporal_pool_rows_arg: bad shape");
  TN_REQUIRE(window >= 1, "tn_temporal_pool_rows_arg: window must be >= 1");
  TN_ON_DEVICE(ctx->device);
  return launch_temporal_pool_rows(feats, rows, feat, idx, samples, window, (int)TN_POOL_MAX, y, ctx->stream, arg);
}

// ---- temporal pooling / PRF1 -------------------------------------------------------
extern "C" int tn_temporal_pool(tn_ctx *ctx, const float *x, int batch, int steps, int feat, tn_pool_kind kind,
                                float *y) {
  TN_REQUIRE(ctx && x && y, "tn_temporal_pool: null argument");
  TN_REQUIRE(batch > 0 && steps > 0 && feat > 0, "tn_temporal_pool: bad shape");
  TN_REQUIRE(kind == TN_POOL_MAX || kind == TN_POOL_MEAN, "tn_temporal_pool: unknown pool kind");
  TN_ON_DEVICE(ctx->device);
  return launch_temporal_pool(x, batch, steps, feat, (int)kind, y, ctx->stream);
}
extern "C" int tn_temporal_pool_arg(tn_ctx *ctx, const float *x, int batch, int steps, int feat, float *y, int32_t *arg) {
  TN_REQUIRE(ctx && x && y && arg, "tn_temporal_pool_arg: null argument");
  TN_REQUIRE(batch > 0 && steps > 0 && feat > 0, "tn_temporal_pool_arg: bad shape");
  TN_ON_DEVICE(ctx->device);
  return launch_pool_max_arg(x, batch, steps, feat, y, arg, ctx->stream);
}

extern "C" int tn_prf1_update(tn_ctx *ctx, const float *logits, const int32_t *labels, int rows, int classes,
                              int64_t *mat) {
  TN_REQUIRE(ctx && logits && labels && mat, "tn_prf1_update: null argument");
  TN_REQUIRE(rows >= 0 && classes > 0, "tn_prf1_update: bad shape");
  if (rows == 0) return TN_OK;
  TN_ON_DEVICE(ctx->device);
  return launch_prf1(logits, labels, rows, classes, mat, ctx->stream);
}
