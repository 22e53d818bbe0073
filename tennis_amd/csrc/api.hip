// C ABI of libtennis_hip.so (see include/tennis_hip.h): error string, context, Dense, bi-RNN and the temporal heads with their
// trainers, temporal pooling and the PRF1 histogram.  The DenseNet-121 frame encoder is encoder.hip.
#include <cmath>
#include <cstdlib>
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
  for (int d = 0; d < 2; ++d) {
    const int rc = launch_transpose_f32(h->w + h->o_wh + (long)d * h->G * h->H * h->H, h->G * h->H, h->H,
                                        h->whT + (long)d * h->H * h->G * h->H, h->ctx->stream);
    if (rc) return rc;
  }
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
  TN_HIP_CHECK(hipMemsetAsync(h->mom, 0, h->n * sizeof(float), ctx->stream));
  TN_HIP_CHECK(hipMemsetAsync(h->g, 0, h->n * sizeof(float), ctx->stream));
  const int rc = head_refresh_whT(h);
  if (rc) return fail(rc);
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
  int rc;
#define TN_TRY(e) do { rc = (e); if (rc) return rc; } while (0)
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
#undef TN_TRY
  if (loss) TN_HIP_CHECK(hipMemcpyAsync(loss, h->loss, sizeof(float) * B, hipMemcpyDeviceToDevice, s));
  if (logits) TN_HIP_CHECK(hipMemcpyAsync(logits, h->logits, sizeof(float) * B * C, hipMemcpyDeviceToDevice, s));
  return TN_OK;
}

extern "C" int tn_head_forward_backward(tn_head *h, const float *x, const int32_t *labels, int B, int T, float *loss,
                                        float *logits) {
  TN_REQUIRE(h && x && labels, "tn_head_forward_backward: null argument");
  TN_REQUIRE(B > 0 && B <= h->maxB && T > 0 && T <= h->maxT, "tn_head_forward_backward: batch / steps exceed the maxima");
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
  TN_REQUIRE(B > 0 && B <= h->maxB && T > 0 && T <= h->maxT, "tn_head_forward_backward_rows: batch / steps exceed the maxima");
  TN_ON_DEVICE(h->ctx->device);
  return head_step(h, nullptr, row_idx, labels, B, T, loss, logits, nullptr, 0);
}

extern "C" int tn_head_forward_rows(tn_head *h, const int32_t *row_idx, int B, int T, float *logits) {
  TN_REQUIRE(h && row_idx && logits, "tn_head_forward_rows: null argument");
  TN_REQUIRE(h->feats, "tn_head_forward_rows: no feature table (call tn_head_set_features first)");
  TN_REQUIRE(B > 0 && B <= h->maxB && T > 0 && T <= h->maxT, "tn_head_forward_rows: batch / steps exceed the maxima");
  TN_ON_DEVICE(h->ctx->device);
  return head_step(h, nullptr, row_idx, nullptr, B, T, nullptr, logits, nullptr, 0);
}

extern "C" int tn_head_buffers(tn_head *h, float **params_dev, float **grads_dev, int64_t *numel) {
  return train_buffers("tn_head_buffers", h, params_dev, grads_dev, numel);
}

// the update alone; scale non-null: the clipped form, on the scale of a reduction the caller has queued
static int head_sgd_update(tn_head *h, float lr, float momentum, float wd, float rescale_grad, const float *scale) {
  int rc = launch_sgd_momentum(h->w, h->g, h->mom, h->n, lr, momentum, wd, rescale_grad, h->ctx->stream, scale);
  if (rc) return rc;
  return head_refresh_whT(h);
}

extern "C" int tn_head_sgd_step(tn_head *h, float lr, float momentum, float wd, float rescale_grad) {
  TN_REQUIRE(h, "tn_head_sgd_step: null handle");
  TN_ON_DEVICE(h->ctx->device);
  if (!h->clip.on()) return head_sgd_update(h, lr, momentum, wd, rescale_grad, nullptr);
  if (int rc = h->clip.reduce(h->ctx, h->g, h->n, nullptr, 0, rescale_grad)) return rc;
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

// ---- end-to-end CNN-RNN training step -------------------------------------------------
// reference train.py:197-236 (--window > 1 --temp_pool gru|lstm, no --feats_model): the fine-tuning step's backbone
// (finetune.hip, built without its classifier) over the batch*steps frames, the temporal head above on its features.
struct tn_cnnrnn_trainer {
  tn_ctx *ctx;
  tn_finetune *bb;
  tn_head *head;
  int B, T, H, W, F;
  bool frozen;
  std::string bb_prefix, rnn_prefix, dense_prefix;
  GradClip clip;                // one norm over backbone + head, one scale for both updates
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
  long fit = -1;
  tn_finetune *bb = nullptr;
  int rc = ft_create(ctx, params, n_params, backbone_prefix, nullptr, height, width, 0, batch * steps, &bb, &fit);
  if (rc == TN_ERR_NOMEM && fit >= 0) {
    tn_set_error("tn_cnnrnn_trainer_create: " + std::to_string((long)batch * steps) + " frames (batch x steps) of " +
                 std::to_string(height) + "x" + std::to_string(width) + " do not fit the device; about " + std::to_string(fit) +
                 " would");
    return rc;
  }
  if (rc) return rc;
  tn_head *head = nullptr;
  rc = tn_head_create(ctx, kind, ft_feature_dim(bb), hidden, classes, params, n_params, rnn_prefix, dense_prefix, batch, steps, &head);
  if (rc) { tn_finetune_destroy(bb); return rc; }
  tn_cnnrnn_trainer *t = new tn_cnnrnn_trainer();
  t->ctx = ctx; t->bb = bb; t->head = head; t->B = batch; t->T = steps; t->H = height; t->W = width; t->F = ft_feature_dim(bb);
  t->frozen = freeze_backbone != 0;
  t->bb_prefix = backbone_prefix; t->rnn_prefix = rnn_prefix; t->dense_prefix = dense_prefix;
  *out = t;
  return TN_OK;
}

// backbone forward (training-mode BatchNorm over all batch*steps frames) -> features (rows b*steps + t) -> head forward / backward
// -> dX straight into the backbone's feature gradient -> backbone backward; frozen: no dX, no backbone backward.  Either way the
// BatchNorm running statistics are updated from the batch statistics (the one place that decides it: docs/numerics.md).
extern "C" int tn_cnnrnn_trainer_forward_backward(tn_cnnrnn_trainer *t, const float *x, const int32_t *labels, int batch, int steps,
                                                  int height, int width, float *loss, float *logits) {
  TN_REQUIRE(t && x && labels, "tn_cnnrnn_trainer_forward_backward: null argument");
  TN_REQUIRE(batch == t->B && steps == t->T,
             "tn_cnnrnn_trainer_forward_backward: batch and steps must equal the handle's (batch x steps frames, BatchNorm statistics over all)");
  TN_REQUIRE(height == t->H && width == t->W, "tn_cnnrnn_trainer_forward_backward: the frame size must equal the handle's");
  TN_ON_DEVICE(t->ctx->device);
  int rc;
#define TN_TRY(e) do { rc = (e); if (rc) return rc; } while (0)
  TN_TRY(ft_forward_features(t->bb, x, t->B * t->T));
  TN_TRY(head_step(t->head, ft_features(t->bb), nullptr, labels, t->B, t->T, loss, logits, t->frozen ? nullptr : ft_feature_grad(t->bb), t->F));
  if (!t->frozen) TN_TRY(ft_backward_features(t->bb, t->B * t->T));
  ft_update_running(t->bb);
#undef TN_TRY
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

extern "C" int tn_cnnrnn_trainer_buffers(tn_cnnrnn_trainer *t, float **backbone_params, float **backbone_grads, int64_t *backbone_numel,
                                         float **head_params, float **head_grads, int64_t *head_numel) {
  TN_REQUIRE(t, "tn_cnnrnn_trainer_buffers: null handle");
  if (int rc = tn_finetune_buffers(t->bb, backbone_params, backbone_grads, backbone_numel)) return rc;
  return tn_head_buffers(t->head, head_params, head_grads, head_numel);
}

extern "C" int tn_cnnrnn_trainer_sgd_step(tn_cnnrnn_trainer *t, float lr, float momentum, float wd, float rescale_grad) {
  TN_REQUIRE(t, "tn_cnnrnn_trainer_sgd_step: null handle");
  TN_ON_DEVICE(t->ctx->device);
  const float *scale = nullptr;
  if (t->clip.on()) {                                      // frozen: the backbone's gradient is no part of the norm
    float *bg = nullptr;
    int64_t bn = 0;
    if (!t->frozen) if (int rc = tn_finetune_buffers(t->bb, nullptr, &bg, &bn)) return rc;
    if (int rc = t->clip.reduce(t->ctx, bg, bn, t->head->g, t->head->n, rescale_grad)) return rc;
    scale = t->clip.scale();
  }
  if (!t->frozen) {                                        // frozen: the backbone's parameters are not touched (grad_req 'null')
    const int rc = ft_sgd_update(t->bb, lr, momentum, wd, rescale_grad, scale);
    if (rc) return rc;
  }
  return head_sgd_update(t->head, lr, momentum, wd, rescale_grad, scale);
}

extern "C" int tn_cnnrnn_trainer_set_clip(tn_cnnrnn_trainer *t, float max_norm) {
  TN_REQUIRE(t, "tn_cnnrnn_trainer_set_clip: null handle");
  return t->clip.set("tn_cnnrnn_trainer_set_clip", t->ctx, max_norm);
}
extern "C" int tn_cnnrnn_trainer_clip_stats(tn_cnnrnn_trainer *t, float *norm, float *scale, int64_t *clipped_steps) {
  TN_REQUIRE(t, "tn_cnnrnn_trainer_clip_stats: null handle");
  return t->clip.stats("tn_cnnrnn_trainer_clip_stats", t->ctx, norm, scale, clipped_steps);
}

extern "C" int tn_cnnrnn_trainer_read_param(tn_cnnrnn_trainer *t, const char *name, int gradient, float *out_host, int64_t capacity,
                                            int64_t *numel) {
  TN_REQUIRE(t && name && out_host && numel, "tn_cnnrnn_trainer_read_param: null argument");
  const std::string n(name);
  if (n.rfind(t->rnn_prefix, 0) == 0 || n.rfind(t->dense_prefix, 0) == 0)
    return tn_head_read_param(t->head, name, gradient, out_host, capacity, numel);
  TN_REQUIRE(n.rfind(t->bb_prefix, 0) == 0, "tn_cnnrnn_trainer_read_param: unknown parameter name");
  return tn_finetune_read_param(t->bb, name, gradient, out_host, capacity, numel);
}

extern "C" int tn_cnnrnn_trainer_set_matmul(tn_cnnrnn_trainer *t, int mode) {
  TN_REQUIRE(t, "tn_cnnrnn_trainer_set_matmul: null handle");
  return tn_finetune_set_matmul(t->bb, mode);
}
extern "C" int tn_cnnrnn_trainer_matmul_stats(tn_cnnrnn_trainer *t, int64_t *f32_launches, int64_t *fp32x3_launches) {
  TN_REQUIRE(t, "tn_cnnrnn_trainer_matmul_stats: null handle");
  return tn_finetune_matmul_stats(t->bb, f32_launches, fp32x3_launches);
}

extern "C" int tn_cnnrnn_trainer_destroy(tn_cnnrnn_trainer *t) {
  if (!t) return TN_OK;
  tn_head_destroy(t->head);                    // (each drains the one stream)
  tn_finetune_destroy(t->bb);
  {
    TnDeviceGuard tn_dg_(t->ctx->device);
    t->clip.release();
  }
  delete t;
  return TN_OK;
}

// ---- end-to-end frame-mode captioner training step ------------------------------------
// reference train_gnmt.py:148-203 without --feats_model: src_embed = TimeDistributed(FrameModel(DenseNet121.features).backbone)
// inside the NMTModel, trained (or frozen, :164-166) by the same loss.backward() / trainer.step(1) (:334-337).  The fine-tuning
// step's backbone (finetune.hip, no classifier) over the batch * steps frames of the padded clips, the captioner's step
// (captioner_train.hip) on its features.
struct tn_gnmt_frames_trainer {
  tn_ctx *ctx;
  tn_finetune *bb;
  tn_gnmt_trainer *cap;
  int side, F, maxB, maxT, maxN;
  long step;                    // Adam's update count, one for both parts
  bool frozen;
  std::string bb_prefix, prefix;
  GradClip clip;                // one norm over backbone + captioner, one scale for both updates
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
  long fit = -1;
  tn_finetune *bb = nullptr;
  int rc = ft_create(ctx, params, n_params, backbone_prefix, nullptr, side, side, 0, max_frames, &bb, &fit);
  if (rc == TN_ERR_NOMEM && fit >= 0) {
    tn_set_error("tn_gnmt_frames_trainer_create: " + std::to_string(max_frames) + " frames (the longest padded batch, batch x steps) of " +
                 std::to_string(side) + "x" + std::to_string(side) + " do not fit the device; about " + std::to_string(fit) + " would");
    return rc;
  }
  if (rc) return rc;
  const int F = ft_feature_dim(bb), G = cell_kind == TN_RNN_GRU ? 3 : 4;
  // the captioner's first layer reads the backbone's features: refuse parameters made for another width
  const std::string w0 = std::string(prefix) + (num_bi_layers > 0 ? "enc_rnn0_l_i2h_weight" : "enc_rnn0_i2h_weight");
  const int64_t w0_numel = ParamMap(params, n_params).numel(w0);
  if (w0_numel >= 0 && w0_numel != (int64_t)G * hidden * F) {
    tn_set_error("tn_gnmt_frames_trainer_create: " + w0 + " is not (gates * hidden, " + std::to_string(F) + "), the backbone's feature width");
    tn_finetune_destroy(bb);
    return TN_ERR_INVALID;
  }
  tn_gnmt_trainer *cap = nullptr;
  rc = tn_gnmt_trainer_create_ex(ctx, params, n_params, prefix, cell_kind, F, hidden, embed, vocab, num_layers, num_bi_layers, flags,
                                 max_batch, max_src_len, max_tgt_len, &cap);
  if (!rc && !freeze_backbone) rc = ft_enable_adam(bb);
  if (rc) { tn_gnmt_trainer_destroy(cap); tn_finetune_destroy(bb); return rc; }
  tn_gnmt_frames_trainer *t = new tn_gnmt_frames_trainer();
  t->ctx = ctx; t->bb = bb; t->cap = cap; t->side = side; t->F = F; t->maxB = max_batch; t->maxT = max_src_len; t->maxN = max_frames;
  t->step = 0; t->frozen = freeze_backbone != 0; t->bb_prefix = backbone_prefix; t->prefix = prefix;
  *out = t;
  return TN_OK;
}

// frames into the handle's staging buffer, zeros in the padded slots -> backbone forward (training-mode BatchNorm over all batch * steps frames, the padded ones
// included: TimeDistributed sends them through with the others) -> features, rows b * steps + t = the captioner's (batch, steps, F)
// source as it stands -> captioner forward / backward, d loss / d src straight into the backbone's feature gradient -> backbone
// backward; frozen: no source gradient, no backbone backward.  Either way the running statistics move (docs/numerics.md).
extern "C" int tn_gnmt_frames_trainer_forward_backward(tn_gnmt_frames_trainer *t, const float *frames, const int32_t *src_valid_len,
                                                       const int32_t *tgt, int ld, const int32_t *tgt_valid_len, int batch, int steps,
                                                       int tgt_len, float *loss, float *logits_out) {
  TN_REQUIRE(t && frames && src_valid_len && tgt && tgt_valid_len && loss, "tn_gnmt_frames_trainer_forward_backward: null argument");
  TN_REQUIRE(batch > 0 && batch <= t->maxB, "tn_gnmt_frames_trainer_forward_backward: batch exceeds max_batch");
  TN_REQUIRE(steps > 0 && steps <= t->maxT, "tn_gnmt_frames_trainer_forward_backward: steps exceed max_src_len");
  TN_REQUIRE((long)batch * steps <= t->maxN, "tn_gnmt_frames_trainer_forward_backward: batch * steps exceeds max_frames");
  TN_REQUIRE(tgt_len >= 2 && ld >= tgt_len, "tn_gnmt_frames_trainer_forward_backward: need tgt_len >= 2 and ld >= tgt_len");
  TN_ON_DEVICE(t->ctx->device);
  const int n = batch * steps;
  int rc;
#define TN_TRY(e) do { rc = (e); if (rc) return rc; } while (0)
  float *x = ft_frame_staging(t->bb);
  TN_TRY(launch_stage_frames(frames, src_valid_len, batch, steps, (long)t->side * t->side * 3, x, t->ctx->stream));
  TN_TRY(ft_forward_features(t->bb, x, n));
  TN_TRY(gnmt_trainer_step(t->cap, ft_features(t->bb), src_valid_len, tgt, ld, tgt_valid_len, batch, steps, tgt_len, loss, logits_out,
                           t->frozen ? nullptr : ft_feature_grad(t->bb), t->F));
  if (!t->frozen) TN_TRY(ft_backward_features(t->bb, n));
  ft_update_running(t->bb);
#undef TN_TRY
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

extern "C" int tn_gnmt_frames_trainer_buffers(tn_gnmt_frames_trainer *t, float **backbone_params, float **backbone_grads,
                                              int64_t *backbone_numel, float **params_dev, float **grads_dev, int64_t *numel) {
  TN_REQUIRE(t, "tn_gnmt_frames_trainer_buffers: null handle");
  if (int rc = tn_finetune_buffers(t->bb, backbone_params, backbone_grads, backbone_numel)) return rc;
  return tn_gnmt_trainer_buffers(t->cap, params_dev, grads_dev, numel);
}

extern "C" int tn_gnmt_frames_trainer_set_dropout(tn_gnmt_frames_trainer *t, float p, uint64_t seed) {
  TN_REQUIRE(t, "tn_gnmt_frames_trainer_set_dropout: null handle");
  return tn_gnmt_trainer_set_dropout(t->cap, p, seed);
}

// gluon.Trainer(model.collect_params(), 'adam').step(1) (train_gnmt.py:310,337) over both parts with one update count; frozen: the
// backbone's parameters have grad_req 'null' (:164-166) and are not touched
extern "C" int tn_gnmt_frames_trainer_adam_step(tn_gnmt_frames_trainer *t, float lr, float beta1, float beta2, float epsilon) {
  TN_REQUIRE(t, "tn_gnmt_frames_trainer_adam_step: null handle");
  TN_ON_DEVICE(t->ctx->device);
  const float *scale = nullptr;
  if (t->clip.on()) {                                      // frozen: the backbone's gradient is no part of the norm
    float *bg = nullptr, *cg = nullptr;
    int64_t bn = 0, cn = 0;
    if (!t->frozen) if (int rc = tn_finetune_buffers(t->bb, nullptr, &bg, &bn)) return rc;
    if (int rc = tn_gnmt_trainer_buffers(t->cap, nullptr, &cg, &cn)) return rc;
    if (int rc = t->clip.reduce(t->ctx, bg, bn, cg, cn, 1.f)) return rc;
    scale = t->clip.scale();
  }
  t->step += 1;
  if (!t->frozen) {
    const int rc = ft_adam_step(t->bb, lr, beta1, beta2, epsilon, t->step, scale);
    if (rc) return rc;
  }
  return gnmt_trainer_adam(t->cap, lr, beta1, beta2, epsilon, t->step, scale);
}

extern "C" int tn_gnmt_frames_trainer_set_clip(tn_gnmt_frames_trainer *t, float max_norm) {
  TN_REQUIRE(t, "tn_gnmt_frames_trainer_set_clip: null handle");
  return t->clip.set("tn_gnmt_frames_trainer_set_clip", t->ctx, max_norm);
}
extern "C" int tn_gnmt_frames_trainer_clip_stats(tn_gnmt_frames_trainer *t, float *norm, float *scale, int64_t *clipped_steps) {
  TN_REQUIRE(t, "tn_gnmt_frames_trainer_clip_stats: null handle");
  return t->clip.stats("tn_gnmt_frames_trainer_clip_stats", t->ctx, norm, scale, clipped_steps);
}

extern "C" int tn_gnmt_frames_trainer_read_param(tn_gnmt_frames_trainer *t, const char *name, int gradient, float *out_host,
                                                 int64_t capacity, int64_t *numel) {
  TN_REQUIRE(t && name && out_host && numel, "tn_gnmt_frames_trainer_read_param: null argument");
  const std::string n(name);
  if (n.rfind(t->bb_prefix, 0) == 0) return tn_finetune_read_param(t->bb, name, gradient, out_host, capacity, numel);
  TN_REQUIRE(n.rfind(t->prefix, 0) == 0, "tn_gnmt_frames_trainer_read_param: unknown parameter name");
  return tn_gnmt_trainer_read_param(t->cap, name, gradient, out_host, capacity, numel);
}

extern "C" int tn_gnmt_frames_trainer_set_matmul(tn_gnmt_frames_trainer *t, int mode) {
  TN_REQUIRE(t, "tn_gnmt_frames_trainer_set_matmul: null handle");
  return tn_finetune_set_matmul(t->bb, mode);
}
extern "C" int tn_gnmt_frames_trainer_matmul_stats(tn_gnmt_frames_trainer *t, int64_t *f32_launches, int64_t *fp32x3_launches) {
  TN_REQUIRE(t, "tn_gnmt_frames_trainer_matmul_stats: null handle");
  return tn_finetune_matmul_stats(t->bb, f32_launches, fp32x3_launches);
}

extern "C" int tn_gnmt_frames_trainer_destroy(tn_gnmt_frames_trainer *t) {
  if (!t) return TN_OK;
  tn_gnmt_trainer_destroy(t->cap);             // (each drains the one stream)
  tn_finetune_destroy(t->bb);
  {
    TnDeviceGuard tn_dg_(t->ctx->device);
    t->clip.release();
  }
  delete t;
  return TN_OK;
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
