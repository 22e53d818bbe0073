// What the handles of api.hip, train_steps.hip, encoder.hip, finetune.hip, captioner.hip and captioner_train.hip share on the host: the device allocations of a handle
// (DevPool), the lookup of its parameters by name and the table of where each lives (param_table.h), and - for the training
// handles - the flat buffers with the one read-back and the one buffers query that go through that table (TrainParams).
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "common.h"
#include "param_table.h"
#include "train.h"

struct DevPool {  // owns device allocations of one handle
  std::vector<void *> ptrs;
  size_t bytes = 0;
  bool failed = false;
  bool dry = false;  // count the bytes only (what a handle would need), allocate nothing
  void *alloc(size_t n) {  // n bytes
    bytes += n;
    if (dry) return nullptr;
    void *p = nullptr;
    if (hipMalloc(&p, n ? n : 16) != hipSuccess) { failed = true; return nullptr; }
    ptrs.push_back(p);
    return p;
  }
  template <typename T>
  T *alloc(size_t n) {  // n elements; a request for none counts, and is, one element
    return (T *)alloc((n ? n : 1) * sizeof(T));
  }
  template <typename T>
  T *upload(const T *h, size_t n) {
    T *d = (T *)alloc(n * sizeof(T));
    if (d && hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { failed = true; return nullptr; }
    return d;
  }
  template <typename T>
  T *upload(const std::vector<T> &h) { return upload(h.data(), h.size()); }
  void release() {
    for (void *p : ptrs) (void)hipFree(p);
    ptrs.clear();
  }
};

// The Dense handle (api.hip); encoder.hip reads its weights for the class activation maps.
struct tn_dense {
  tn_ctx *ctx;
  DevPool pool;
  float *w, *b;      // (units, in_units), (units) or nullptr: fp32 on the device
  int units, in_units;
};

// tn_birnn_forward (api.hip) with its input never materialised: row b * steps + t of x is row row_idx[b * steps + t] of table (n_rows,
// input_size; row stride ld, DEVICE), a row of zeros where the index is negative; what tn_gnmt_encode_rows runs for encoder layer 0.
int birnn_forward_rows(tn_birnn *r, const float *table, int n_rows, int ld, const int32_t *row_idx, int batch, int steps,
                       const int32_t *valid_len, float *seq, float *h_last, float *c_last);

// Global-norm gradient clipping of one training handle (tn_<handle>_set_clip / _clip_stats, tennis_hip.h): the threshold on the
// host, the reduction's workspace and the record on the device, allocated when clipping is first switched on.  A step with
// clipping on calls reduce() over its trainable gradient buffer(s) and hands scale() to launch_sgd_momentum / launch_adam.
struct GradClip {
  float max_norm = 0.f;             // 0: off
  long steps = 0;                   // steps taken with clipping on
  float *partials = nullptr;        // TN_GRAD_SUMSQ_GRID floats, the record behind them (one allocation)
  tn_clip_record *rec = nullptr;
  bool on() const { return max_norm > 0.f; }
  const float *scale() const { return &rec->scale; }
  int set(const char *fn, tn_ctx *ctx, float v) {
    TN_REQUIRE(std::isfinite(v) && v >= 0.f, std::string(fn) + ": max_norm must be finite and >= 0 (0 switches clipping off)");
    if (v > 0.f && !partials) {
      TN_ON_DEVICE(ctx->device);
      void *p = nullptr;
      const size_t ws = sizeof(float) * TN_GRAD_SUMSQ_GRID;
      if (hipMalloc(&p, ws + sizeof(tn_clip_record)) != hipSuccess) { tn_set_error("device allocation failed"); return TN_ERR_NOMEM; }
      partials = (float *)p;
      rec = (tn_clip_record *)((char *)p + ws);
      TN_HIP_CHECK(hipMemsetAsync(rec, 0, sizeof(tn_clip_record), ctx->stream));
    }
    max_norm = v;
    return TN_OK;
  }
  // a, b: the trainable gradient segments of this step (b may be empty); rescale: the step's rescale_grad
  int reduce(tn_ctx *ctx, const float *a, long na, const float *b, long nb, float rescale) {
    if (int rc = launch_grad_sumsq(a, na, b, nb, rescale, max_norm, partials, rec, ctx->stream)) return rc;
    ++steps;
    return TN_OK;
  }
  int stats(const char *fn, tn_ctx *ctx, float *norm, float *scale, int64_t *clipped_steps) {
    TN_REQUIRE(on(), std::string(fn) + ": clipping is off (set_clip first)");
    TN_REQUIRE(steps > 0, std::string(fn) + ": no step has run with clipping on");
    TN_ON_DEVICE(ctx->device);
    tn_clip_record r;
    TN_HIP_CHECK(hipMemcpyAsync(&r, rec, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
    TN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (norm) *norm = r.norm;
    if (scale) *scale = r.scale;
    if (clipped_steps) *clipped_steps = r.clipped;
    return TN_OK;
  }
  void release() {          // after the stream has drained
    if (partials) (void)hipFree(partials);
    partials = nullptr; rec = nullptr;
  }
};

// The head of every training handle (tn_head, tn_finetune, tn_gnmt_trainer): the flat parameter / gradient buffers, the state
// buffer of the handles that have one, and the table that names their contents.
struct TrainParams {
  tn_ctx *ctx = nullptr;
  DevPool pool;
  ParamTable table;
  long n = 0;                 // parameters in the flat buffers (= table.n)
  float *w = nullptr, *g = nullptr, *state = nullptr;
  GradClip clip;              // off after create
};

// *_read_param of a training handle: the named parameter (a convolution weight back in (O, I, kh, kw) order), its gradient
// (gradient = 1; state and pointer rows have none and read the same either way) into out_host.  fn: the caller's name, for the errors.
inline int train_read_param(const char *fn, TrainParams *h, const char *name, int gradient, float *out_host, int64_t capacity,
                            int64_t *numel) {
  TN_REQUIRE(h && name && out_host && numel, std::string(fn) + ": null argument");
  const ParamTable::Row *r = h->table.find(name);
  TN_REQUIRE(r && (r->where != ParamTable::PTR || r->ptr), std::string(fn) + ": unknown parameter name");
  TN_REQUIRE(capacity >= r->count, std::string(fn) + ": host buffer too small");
  TN_ON_DEVICE(h->ctx->device);
  TN_HIP_CHECK(hipStreamSynchronize(h->ctx->stream));
  const float *dev = r->where == ParamTable::PTR ? r->ptr : (r->where == ParamTable::STATE ? h->state : gradient ? h->g : h->w) + r->off;
  if (r->O) {
    std::vector<float> tmp(r->count);
    TN_HIP_CHECK(hipMemcpy(tmp.data(), dev, sizeof(float) * r->count, hipMemcpyDeviceToHost));
    conv_from_gemm(tmp.data(), out_host, r->O, r->I, r->kh, r->kw);
  } else {
    TN_HIP_CHECK(hipMemcpy(out_host, dev, sizeof(float) * r->count, hipMemcpyDeviceToHost));
  }
  *numel = r->count;
  return TN_OK;
}

inline int train_buffers(const char *fn, TrainParams *h, float **params_dev, float **grads_dev, int64_t *numel) {
  TN_REQUIRE(h, std::string(fn) + ": null handle");
  if (params_dev) *params_dev = h->w;
  if (grads_dev) *grads_dev = h->g;
  if (numel) *numel = h->n;
  return TN_OK;
}
