// Test / tuning hooks: run a single encoder kernel on caller-provided device
// buffers so the -m gpu parity tests can pin each kernel against the oracle on
// its own (ragged M, channel offsets) and scripts/kbench.py can time one kernel
// at one layer shape.  Host-weight variants fold/pack exactly as
// tn_densenet121_create does.
#include <cstring>
#include <vector>

#include "common.h"
#include "encoder_plan.h"
#include "gemm_fp32x3.h"
#include "gnmt_kernels.h"
#include "linear.h"
#include "param_table.h"
#include "rnn.h"
#include "train.h"

namespace {
template <typename T>
T *up(const std::vector<T> &h) {
  T *d = nullptr;
  if (hipMalloc(&d, h.size() * sizeof(T)) != hipSuccess) return nullptr;
  if (hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  return d;
}
}  // namespace

std::vector<f16> pack_conv3x3(const float *w);  // encoder.hip

// fp32 (32,128,3,3) -> the packed fp16 fragment image the conv3x3 kernel consumes (72*64*8 halfs).
extern "C" int tn_dbg_pack_conv3x3(const float *w_host, uint16_t *out_host) {
  TN_REQUIRE(w_host && out_host, "tn_dbg_pack_conv3x3: null argument");
  const std::vector<f16> p = pack_conv3x3(w_host);
  memcpy(out_host, p.data(), p.size() * sizeof(f16));
  return TN_OK;
}

// Asynchronous single launches on device-resident operands (weights already fp16 / packed).
extern "C" int tn_dbg_conv1x1_dev(tn_ctx *ctx, const void *x_f16, int ldx, int K, const float *scale,
                                  const float *shift, const void *w_f16, int N, void *y_f16, int ldy, int yoff, int M,
                                  int pool, int H, int W, int variant) {
  TN_REQUIRE(ctx && x_f16 && y_f16 && scale && shift && w_f16, "tn_dbg_conv1x1_dev: null argument");
  Conv1x1Args a{(const f16 *)x_f16, ldx, K, scale, shift, (const f16 *)w_f16, N, (f16 *)y_f16, ldy, yoff, M, pool, H, W};
  a.variant = variant & 0xffff;
  a.exact = (variant >> 17) & 1;      // bit 17: w is [N][2 K] = [hi | lo] (exact-weights mode)
  if ((variant >> 18) & 1) {          // bit 18: the warp-specialised transition kernel (trans_ws.hip); the fragment image of w is built per call
    TN_REQUIRE(trans_ws_supported(a), "tn_dbg_conv1x1_dev: geometry not supported by trans_ws");
    TN_ON_DEVICE(ctx->device);
    static f16 *frags[64] = {};             // (a test hook: one scratch image per device, grown on demand, never freed; not thread-safe)
    static size_t frag_halves[64] = {};
    TN_REQUIRE(ctx->device >= 0 && ctx->device < 64, "tn_dbg_conv1x1_dev: device index out of range");
    f16 *&frag = frags[ctx->device];
    if (frag_halves[ctx->device] < (size_t)N * K) {
      if (frag) (void)hipFree(frag);
      frag = nullptr; frag_halves[ctx->device] = 0;
      TN_HIP_CHECK(hipMalloc((void **)&frag, (size_t)N * K * sizeof(f16)));
      frag_halves[ctx->device] = (size_t)N * K;
    }
    const int rc = launch_pack_trans_frags(a.w, N, K, frag, ctx->stream);
    if (rc) return rc;
    a.wfrag = frag;
  }
  return launch_conv1x1(a, ctx->stream);
}

// tn_dbg_conv1x1_dev with every argument of Conv1x1Args a test has to reach: bias (device fp32 [N], or NULL), clamp (scale / shift hold
// lo / hi), y32 / ld32 (the fp32 side output, or NULL) and wfrag - the CALLER's fragment image of w (device; what pack_trans_frags made
// of it on the host, as tn_densenet121_create does, or launch_pack_trans_frags on the device), or NULL.  variant: bit 17 exact weights.
// Asynchronous.
extern "C" int tn_dbg_conv1x1_ex(tn_ctx *ctx, const void *x_f16, int ldx, int K, const float *scale, const float *shift, const void *w_f16,
                                 int N, void *y_f16, int ldy, int yoff, int M, int pool, int H, int W, int variant, const float *bias,
                                 int clamp, float *y32, int ld32, const void *wfrag) {
  TN_REQUIRE(ctx && x_f16 && y_f16 && scale && shift && w_f16, "tn_dbg_conv1x1_ex: null argument");
  TN_REQUIRE(M > 0 && K > 0 && N > 0 && ldx >= K && ldy >= yoff + N && yoff >= 0, "tn_dbg_conv1x1_ex: bad shape (M, K, N positive, ldx >= K, ldy >= yoff + N)");
  TN_REQUIRE(!pool || (H >= 2 && W >= 2 && M % ((H / 2) * (W / 2)) == 0), "tn_dbg_conv1x1_ex: pooling needs H, W >= 2 and M = B (H / 2) (W / 2)");
  TN_REQUIRE(!y32 || (ld32 >= N && ld32 % 4 == 0 && ((uintptr_t)y32 & 15) == 0), "tn_dbg_conv1x1_ex: y32 needs ld32 >= N, a multiple of 4, and 16-byte alignment");
  Conv1x1Args a{(const f16 *)x_f16, ldx, K, scale, shift, (const f16 *)w_f16, N, (f16 *)y_f16, ldy, yoff, M, pool, H, W};
  a.variant = variant & 0xffff;
  a.exact = (variant >> 17) & 1;
  a.bias = bias;
  a.clamp = clamp != 0;
  a.y32 = y32;
  a.ld32 = ld32;
  a.wfrag = (const f16 *)wfrag;
  TN_REQUIRE(!wfrag || trans_ws_supported(a), "tn_dbg_conv1x1_ex: wfrag with a geometry trans_ws does not support (pooling, fp16 weights, no bias, N = 512 | 256, K % 128 == 0, even H and W)");
  TN_ON_DEVICE(ctx->device);
  return launch_conv1x1(a, ctx->stream);
}

// tn_dbg_conv1x1_ex with the head epilogue of the warp-specialised transition (trans_ws.hip, round 10): feat (device fp32, row pitch
// ldfeat) receives, per frame, the mean over the frame's pooled pixels of relu(head_s[n] * result + head_t[n]) for n in [0, N);
// head_s / head_t device fp32 [N].  y32 has to be NULL or is left untouched.  The launcher refuses what the epilogue does not
// cover (anything but wfrag, N = 512 and a 14 x 14 map), before any launch.  Asynchronous.
extern "C" int tn_dbg_conv1x1_head(tn_ctx *ctx, const void *x_f16, int ldx, int K, const float *scale, const float *shift, const void *w_f16,
                                   int N, void *y_f16, int ldy, int yoff, int M, int pool, int H, int W, float *y32, int ld32, const void *wfrag,
                                   float *feat, const float *head_s, const float *head_t, int ldfeat) {
  TN_REQUIRE(ctx && x_f16 && y_f16 && scale && shift && w_f16 && wfrag && feat && head_s && head_t, "tn_dbg_conv1x1_head: null argument");
  TN_REQUIRE(M > 0 && K > 0 && N > 0 && ldx >= K && ldy >= yoff + N && yoff >= 0 && ldfeat >= N, "tn_dbg_conv1x1_head: bad shape (M, K, N positive, ldx >= K, ldy >= yoff + N, ldfeat >= N)");
  TN_REQUIRE(pool && H >= 2 && W >= 2 && M % ((H / 2) * (W / 2)) == 0, "tn_dbg_conv1x1_head: a pooling transition with M = B (H / 2) (W / 2)");
  TN_REQUIRE(!y32 || (ld32 >= N && ld32 % 4 == 0 && ((uintptr_t)y32 & 15) == 0), "tn_dbg_conv1x1_head: y32 needs ld32 >= N, a multiple of 4, and 16-byte alignment");
  Conv1x1Args a{(const f16 *)x_f16, ldx, K, scale, shift, (const f16 *)w_f16, N, (f16 *)y_f16, ldy, yoff, M, pool, H, W};
  a.y32 = y32;
  a.ld32 = ld32;
  a.wfrag = (const f16 *)wfrag;
  a.feat = feat; a.head_s = head_s; a.head_t = head_t; a.ldfeat = ldfeat;
  TN_REQUIRE(trans_ws_supported(a), "tn_dbg_conv1x1_head: a geometry trans_ws does not support (N = 512 | 256, K % 128 == 0, even H and W)");
  TN_ON_DEVICE(ctx->device);
  return launch_conv1x1(a, ctx->stream);
}

// The two forms of the warp-specialised transition's weight packer: the host function tn_densenet121_create calls (no device is
// touched) and the device kernel; w [N][K] fp16 -> [K / 16][N / 32][64 lanes][8], N K halves
extern "C" int tn_dbg_pack_trans_frags(const uint16_t *w_f16_host, int N, int K, uint16_t *out_host) {
  TN_REQUIRE(w_f16_host && out_host, "tn_dbg_pack_trans_frags: null argument");
  TN_REQUIRE(N > 0 && K > 0 && N % 32 == 0 && K % 16 == 0, "tn_dbg_pack_trans_frags: N % 32 or K % 16");
  const std::vector<f16> p = pack_trans_frags((const f16 *)w_f16_host, N, K);
  memcpy(out_host, p.data(), p.size() * sizeof(f16));
  return TN_OK;
}
extern "C" int tn_dbg_pack_trans_frags_dev(tn_ctx *ctx, const void *w_f16, int N, int K, void *out_f16) {
  TN_REQUIRE(ctx && w_f16 && out_f16, "tn_dbg_pack_trans_frags_dev: null argument");
  TN_REQUIRE(N > 0 && K > 0, "tn_dbg_pack_trans_frags_dev: N and K must be positive");
  TN_ON_DEVICE(ctx->device);
  return launch_pack_trans_frags((const f16 *)w_f16, N, K, (f16 *)out_f16, ctx->stream);
}

extern "C" int tn_dbg_conv3x3_dev(tn_ctx *ctx, const void *x_f16, const float *scale, const float *shift,
                                  const void *wp_f16, void *y_f16, int ldy, int yoff, int B, int H, int W,
                                  int variant) {
  TN_REQUIRE(ctx && x_f16 && y_f16 && scale && shift && wp_f16, "tn_dbg_conv3x3_dev: null argument");
  Conv3x3Args a{(const f16 *)x_f16, scale, shift, (const f16 *)wp_f16, (f16 *)y_f16, ldy, yoff, B * H * W, H, W};
  a.variant = variant & 0xffff;
  a.exact = (variant >> 17) & 1;      // bit 17: wp is the hi image (both MFMA layouts, tn_dbg_pack_conv3x3) followed by the lo image
  return launch_conv3x3(a, ctx->stream);
}

// y[m][yoff+n] = sum_k relu(scale[k]*x[m][k]+shift[k]) * w[n][k]   (pool: 2x2 mean first)
extern "C" int tn_dbg_conv1x1(tn_ctx *ctx, const void *x_f16, int ldx, int K, const float *scale_host,
                              const float *shift_host, const float *w_host /*[N][K]*/, int N, void *y_f16, int ldy,
                              int yoff, int M, int pool, int H, int W) {
  TN_REQUIRE(ctx && x_f16 && y_f16 && scale_host && shift_host && w_host, "tn_dbg_conv1x1: null argument");
  TN_ON_DEVICE(ctx->device);
  std::vector<f16> wh((size_t)N * K);
  for (size_t i = 0; i < wh.size(); ++i) wh[i] = (f16)w_host[i];
  f16 *w = up(wh);
  float *s = up(std::vector<float>(scale_host, scale_host + K));
  float *t = up(std::vector<float>(shift_host, shift_host + K));
  TN_REQUIRE(w && s && t, "tn_dbg_conv1x1: device allocation failed");
  const int rc = tn_dbg_conv1x1_dev(ctx, x_f16, ldx, K, s, t, w, N, y_f16, ldy, yoff, M, pool, H, W, 0);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(w); (void)hipFree(s); (void)hipFree(t);
  if (rc) return rc;
  TN_HIP_CHECK(e);
  return TN_OK;
}

// y[m][yoff+n] = conv3x3(relu(scale*x+shift), w (32,128,3,3), pad 1) over (B,H,W,128) NHWC
extern "C" int tn_dbg_conv3x3(tn_ctx *ctx, const void *x_f16, const float *scale_host, const float *shift_host,
                              const float *w_host, void *y_f16, int ldy, int yoff, int B, int H, int W) {
  TN_REQUIRE(ctx && x_f16 && y_f16 && scale_host && shift_host && w_host, "tn_dbg_conv3x3: null argument");
  TN_ON_DEVICE(ctx->device);
  f16 *w = up(pack_conv3x3(w_host));
  float *s = up(std::vector<float>(scale_host, scale_host + 128));
  float *t = up(std::vector<float>(shift_host, shift_host + 128));
  TN_REQUIRE(w && s && t, "tn_dbg_conv3x3: device allocation failed");
  const int rc = tn_dbg_conv3x3_dev(ctx, x_f16, s, t, w, y_f16, ldy, yoff, B, H, W, 0);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(w); (void)hipFree(s); (void)hipFree(t);
  if (rc) return rc;
  TN_HIP_CHECK(e);
  return TN_OK;
}

// One fused dense layer in place on buf (B,H,W,ldc): device-resident, pre-converted operands.
extern "C" int tn_dbg_dense_layer_dev(tn_ctx *ctx, void *buf_f16, int ldc, int K, const float *s1, const float *t1,
                                      const void *w1_f16, const float *s2, const float *t2, const void *w3p_f16,
                                      int B, int H, int W, unsigned long long *ts, int variant) {
  TN_REQUIRE(ctx && buf_f16 && s1 && t1 && w1_f16 && s2 && t2 && w3p_f16, "tn_dbg_dense_layer_dev: null argument");
  DenseLayerArgs a{(f16 *)buf_f16, ldc, K, s1, t1, (const f16 *)w1_f16, s2, t2, (const f16 *)w3p_f16, B, H, W};
  a.ts = ts;
  a.variant = variant & 0xffff;
  a.exact = (variant >> 17) & 1;      // bit 17: w1 is [128][2 Kp] = [hi | lo], w3p the hi image followed by the lo image
  return launch_dense_layer(a, ctx->stream);
}

// nchain consecutive fused dense layers (K0, K0 + 32, ...) in place on buf (B,H,W,ldc) as ONE chained launch: the per-layer device
// pointers come as host arrays of nchain entries each; the DenseLayerDev array is built on the device here.  variant as
// tn_dbg_dense_layer_dev (bit 17: exact weights; bit 19: hand the launcher nchain WITHOUT the layer array - a call it has to
// refuse).  Synchronous; frees what it allocates.
extern "C" int tn_dbg_dense_chain_dev(tn_ctx *ctx, void *buf_f16, int ldc, int K0, int nchain, const float *const *s1, const float *const *t1,
                                      const void *const *w1_f16, const float *const *s2, const float *const *t2, const void *const *w3p_f16,
                                      int B, int H, int W, int variant) {
  TN_REQUIRE(ctx && buf_f16 && s1 && t1 && w1_f16 && s2 && t2 && w3p_f16, "tn_dbg_dense_chain_dev: null argument");
  TN_REQUIRE(nchain > 0 && nchain <= 64, "tn_dbg_dense_chain_dev: nchain must be 1 ... 64");
  std::vector<DenseLayerDev> cd(nchain);
  for (int l = 0; l < nchain; ++l) {
    TN_REQUIRE(s1[l] && t1[l] && w1_f16[l] && s2[l] && t2[l] && w3p_f16[l], "tn_dbg_dense_chain_dev: null layer operand");
    cd[l] = DenseLayerDev{s1[l], t1[l], (const f16 *)w1_f16[l], s2[l], t2[l], (const f16 *)w3p_f16[l]};
  }
  TN_ON_DEVICE(ctx->device);
  DenseLayerDev *chain = up(cd);
  TN_REQUIRE(chain, "tn_dbg_dense_chain_dev: device allocation failed");
  DenseLayerArgs a{(f16 *)buf_f16, ldc, K0, cd[0].s1, cd[0].t1, cd[0].w1, cd[0].s2, cd[0].t2, cd[0].w3p, B, H, W};
  a.variant = variant & 0xffff;
  a.exact = (variant >> 17) & 1;
  a.chain = ((variant >> 19) & 1) ? nullptr : chain;
  a.nchain = nchain;
  const int rc = launch_dense_layer(a, ctx->stream);
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(chain);
  if (rc) return rc;
  TN_HIP_CHECK(e);
  return TN_OK;
}

// The calibration statistic of tn_densenet121_input_means on its own: per-channel mean over `rows` rows of x (rows, ld) fp16 of
// relu(scale x + shift), or of clamp(x, lo = scale, hi = shift) with `clamp`; one synchronous launch_channel_mean, all operands
// on the device, the scratch the caller's (scratch_bytes: at least 32 K doubles)
extern "C" int tn_dbg_channel_mean(tn_ctx *ctx, const void *x_f16, int ld, int K, const float *scale, const float *shift, int64_t rows,
                                   void *scratch, size_t scratch_bytes, float *out, int clamp) {
  TN_REQUIRE(ctx && x_f16 && scale && shift && scratch && out, "tn_dbg_channel_mean: null argument");
  TN_REQUIRE(K > 0 && ld >= K && rows > 0, "tn_dbg_channel_mean: bad shape");
  TN_REQUIRE(scratch_bytes >= (size_t)32 * K * sizeof(double), "tn_dbg_channel_mean: scratch smaller than 32 K doubles");
  TN_ON_DEVICE(ctx->device);
  const int rc = launch_channel_mean((const f16 *)x_f16, ld, K, scale, shift, (long)rows, (double *)scratch, out, ctx->stream, clamp != 0);
  if (rc) return rc;
  TN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return TN_OK;
}

// ---- the first and the last kernels of a forward: stem (+ maxpool) and head ----
// The pooled stem map of B frames x (device, in `layout`) into y (device fp16, row stride ldy >= 64): conv0's raw weights (64,3,7,7)
// and batchnorm0's parameters (host fp32) folded by the function tn_densenet121_create folds them with (encoder.hip::fold_stem), then
// the launchers of the forward - fused: launch_stem_pool; otherwise launch_stem into a map of its own + launch_maxpool3x3s2
// (TN_NO_FUSE).  centre_host: m_c of the centred output or NULL (no floor).  Synchronous.
extern "C" int tn_dbg_stem(tn_ctx *ctx, const float *w0_host, const float *gamma_host, const float *beta_host, const float *mean_host,
                           const float *var_host, const float *centre_host, int exact, int fused, int layout, int B, int H, int W,
                           const void *x, void *y_f16, int ldy) {
  TN_REQUIRE(ctx && w0_host && gamma_host && beta_host && mean_host && var_host && x && y_f16, "tn_dbg_stem: null argument");
  TN_REQUIRE(layout >= 0 && layout <= 2, "tn_dbg_stem: unknown input layout");
  TN_REQUIRE(B > 0 && H >= 16 && W >= 16 && H <= 1024 && W <= 1024, "tn_dbg_stem: bad shape (frames of 16 .. 1024 pixels a side)");
  TN_REQUIRE(ldy >= 64 && ldy % 8 == 0, "tn_dbg_stem: the output stride must be a multiple of 8, at least 64");
  TN_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y_f16 & 15) == 0, "tn_dbg_stem: x and y must be 16-byte aligned");
  TN_REQUIRE(fused || !exact, "tn_dbg_stem: the exact-weights mode has the fused kernel only");
  TN_ON_DEVICE(ctx->device);
  const StemFold f = fold_stem_bn(w0_host, gamma_host, beta_host, mean_host, var_host, centre_host, exact != 0);
  const int Ho = (H + 6 - 7) / 2 + 1, Wo = (W + 6 - 7) / 2 + 1, Hp = (Ho + 2 - 3) / 2 + 1, Wp = (Wo + 2 - 3) / 2 + 1;
  f16 *wp = up(f.wp), *wp_zf = up(f.wp_zf), *wp_lo = exact ? up(f.wp_zf_lo) : nullptr, *map = nullptr;
  float *sc = up(f.scale), *sh = up(f.shift), *shu = up(f.shift_u8), *fl = centre_host ? up(f.floor) : nullptr;
  bool ok = wp && wp_zf && sc && sh && shu && (!exact || wp_lo) && (!centre_host || fl);
  if (ok && !fused) ok = hipMalloc((void **)&map, (size_t)B * Ho * Wo * 64 * sizeof(f16)) == hipSuccess;
  int rc = TN_OK;
  if (ok) {
    StemArgs a{x, layout, B, H, W, wp, wp_zf, sc, sh, map, Ho, Wo};
    a.shift_u8 = shu;
    a.wp_zf_lo = wp_lo;
    a.floor = fl;
    if (fused) rc = launch_stem_pool(a, (f16 *)y_f16, ldy, Hp, Wp, ctx->stream);
    else {
      rc = launch_stem(a, ctx->stream);
      if (!rc) rc = launch_maxpool3x3s2(map, B, Ho, Wo, 64, (f16 *)y_f16, ldy, Hp, Wp, ctx->stream);
    }
  }
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(wp); (void)hipFree(wp_zf); (void)hipFree(wp_lo); (void)hipFree(map);
  (void)hipFree(sc); (void)hipFree(sh); (void)hipFree(shu); (void)hipFree(fl);
  TN_REQUIRE(ok, "tn_dbg_stem: device allocation failed");
  if (rc) return rc;
  TN_HIP_CHECK(e);
  return TN_OK;
}

// MaxPool2D(3, 2, pad 1) of a device fp16 NHWC map (B,H,W,C) into y (B,Ho,Wo; row stride ldy): launch_maxpool3x3s2.  Synchronous.
extern "C" int tn_dbg_maxpool(tn_ctx *ctx, const void *x_f16, int B, int H, int W, int C, void *y_f16, int ldy, int Ho, int Wo) {
  TN_REQUIRE(ctx && x_f16 && y_f16, "tn_dbg_maxpool: null argument");
  TN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && ldy >= C, "tn_dbg_maxpool: bad shape");
  TN_REQUIRE(Ho == (H - 1) / 2 + 1 && Wo == (W - 1) / 2 + 1, "tn_dbg_maxpool: the output is ((H - 1) / 2 + 1) x ((W - 1) / 2 + 1)");
  TN_REQUIRE(((uintptr_t)x_f16 & 15) == 0 && ((uintptr_t)y_f16 & 15) == 0, "tn_dbg_maxpool: x and y must be 16-byte aligned");
  TN_ON_DEVICE(ctx->device);
  const int rc = launch_maxpool3x3s2((const f16 *)x_f16, B, H, W, C, (f16 *)y_f16, ldy, Ho, Wo, ctx->stream);
  if (rc) return rc;
  TN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return TN_OK;
}

// BatchNorm + ReLU + AvgPool2D(7) + NCHW flatten of a device NHWC map (B,H,W,C) into feat (B, C PH PW) device fp32: launch_head on the
// fp16 map x_f16, or - x32 non-NULL - on the fp32 side buffer (x_f16 is then not read).  scale / shift device fp32.  Synchronous.
extern "C" int tn_dbg_head(tn_ctx *ctx, const void *x_f16, const float *x32, int B, int H, int W, int C, const float *scale, const float *shift,
                           float *feat, int PH, int PW) {
  TN_REQUIRE(ctx && (x_f16 || x32) && scale && shift && feat, "tn_dbg_head: null argument");
  TN_REQUIRE(B > 0 && C > 0 && PH > 0 && PW > 0 && 7 * PH <= H && 7 * PW <= W, "tn_dbg_head: bad shape (PH x PW windows of 7 x 7 inside H x W)");
  TN_REQUIRE((((uintptr_t)x_f16 | (uintptr_t)x32) & 15) == 0, "tn_dbg_head: the map must be 16-byte aligned");
  TN_ON_DEVICE(ctx->device);
  const int rc = launch_head((const f16 *)x_f16, B, H, W, C, scale, shift, feat, PH, PW, ctx->stream, x32);
  if (rc) return rc;
  TN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return TN_OK;
}

// class_maps_kernel alone (tennis_hip_debug.h): launch_class_maps on the fp16 map x_f16 or - x32 non-NULL - on the fp32 one.  Synchronous.
extern "C" int tn_dbg_class_maps(tn_ctx *ctx, const void *x_f16, const float *x32, int B, int H, int W, int C, const float *scale,
                                 const float *shift, const float *wd, int PH, int PW, int classes, float *maps, int *n_seq, int *depth) {
  TN_REQUIRE(ctx && (x_f16 || x32) && scale && shift && wd && maps, "tn_dbg_class_maps: null argument");
  TN_REQUIRE((((uintptr_t)x_f16 | (uintptr_t)x32 | (uintptr_t)wd) & 15) == 0, "tn_dbg_class_maps: the map and the weights must be 16-byte aligned");
  TN_ON_DEVICE(ctx->device);
  const int rc = launch_class_maps((const f16 *)x_f16, x32, B, H, W, C, scale, shift, wd, PH, PW, classes, maps, ctx->stream);
  if (rc) return rc;
  TN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (n_seq) *n_seq = class_maps_seq(C);
  if (depth) *depth = class_maps_depth();
  return TN_OK;
}

// fp32 linear: y = x W^T + b
extern "C" int tn_dbg_linear(tn_ctx *ctx, const float *x, const float *w, const float *bias, float *y, int M, int N,
                             int K) {
  TN_REQUIRE(ctx && x && w && y, "tn_dbg_linear: null argument");
  TN_ON_DEVICE(ctx->device);
  return launch_linear_f32(x, K, w, K, bias, y, N, M, N, K, 0, ctx->stream);
}

// ---- strip-streaming fused dense layer (dense_strip_impl.h) ----
// fp32 (128,K) 1x1 weights with BN2's folded scale / shift (128 each) and (32,128,3,3) 3x3 weights -> the fragment images the
// strip kernel keeps in LDS ((K+16)*128 and 36864 halfs); the scale is multiplied into the weights before the fp16 rounding
extern "C" int tn_dbg_pack_strip(const float *w1_host, int K, const float *s2_host, const float *t2_host, uint16_t *w1s_out,
                                 const float *w3_host, uint16_t *w3s_out) {
  TN_REQUIRE(K > 0 && K % 32 == 0, "tn_dbg_pack_strip: K must be a multiple of 32");
  if (w1_host && w1s_out) {
    TN_REQUIRE(s2_host && t2_host, "tn_dbg_pack_strip: the 1x1 image needs BN2's scale and shift");
    std::vector<float> wf((size_t)128 * K);
    for (int n = 0; n < 128; ++n)
      for (int k = 0; k < K; ++k) wf[(size_t)n * K + k] = w1_host[(size_t)n * K + k] * s2_host[n];
    const std::vector<f16> p = pack_w1_strip(wf.data(), K, t2_host);
    memcpy(w1s_out, p.data(), p.size() * sizeof(f16));
  }
  if (w3_host && w3s_out) {
    const std::vector<f16> p = pack_w3_strip(w3_host);
    memcpy(w3s_out, p.data(), p.size() * sizeof(f16));
  }
  return TN_OK;
}

// One fused dense layer in place on buf (B,H,W,ldc), asynchronous, device-resident packed operands.
extern "C" int tn_dbg_dense_strip_dev(tn_ctx *ctx, void *buf_f16, int ldc, int K, const float *s1, const float *t1,
                                      const void *w1s_f16, const void *w3s_f16, int B, int H, int W, unsigned long long *ts) {
  TN_REQUIRE(ctx && buf_f16 && s1 && t1 && w1s_f16 && w3s_f16, "tn_dbg_dense_strip_dev: null argument");
  DenseStripArgs a{(f16 *)buf_f16, ldc, K, s1, t1, (const f16 *)w1s_f16, (const f16 *)w3s_f16, B, H, W};
  a.ts = ts;
  return launch_dense_strip(a, ctx->stream);
}

// The same layer in the paired launch geometry (dense_strip_pair_w28.hip: 28 x 28 only, two frames per workgroup, an even B);
// ts: 128 stamps per WORKGROUP (B / 2 of them), wave 0's = the upper half of the workgroup's first frame
extern "C" int tn_dbg_dense_strip_pair_dev(tn_ctx *ctx, void *buf_f16, int ldc, int K, const float *s1, const float *t1,
                                           const void *w1s_f16, const void *w3s_f16, int B, int H, int W, unsigned long long *ts) {
  TN_REQUIRE(ctx && buf_f16 && s1 && t1 && w1s_f16 && w3s_f16, "tn_dbg_dense_strip_pair_dev: null argument");
  DenseStripArgs a{(f16 *)buf_f16, ldc, K, s1, t1, (const f16 *)w1s_f16, (const f16 *)w3s_f16, B, H, W};
  a.ts = ts;
  return launch_dense_strip_pair(a, ctx->stream);
}

// nl layers K0, K0 + 32, ... in one paired launch (dense_strip_pair_kernel_chain: K0 = 128, nl = 6); per-layer operand arrays of
// DEVICE pointers, host-resident.  Synchronous: the layer table is uploaded for the call and freed behind it.
extern "C" int tn_dbg_dense_strip_pair_chain_dev(tn_ctx *ctx, void *buf_f16, int ldc, int K0, int nl, const float *const *s1,
                                                 const float *const *t1, const void *const *w1s_f16, const void *const *w3s_f16, int B,
                                                 int H, int W) {
  TN_REQUIRE(ctx && buf_f16 && s1 && t1 && w1s_f16 && w3s_f16, "tn_dbg_dense_strip_pair_chain_dev: null argument");
  TN_REQUIRE(nl > 0 && nl <= 16, "tn_dbg_dense_strip_pair_chain_dev: bad layer count");
  TN_ON_DEVICE(ctx->device);
  std::vector<DenseStripLayerDev> tab(nl);
  for (int l = 0; l < nl; ++l) {
    TN_REQUIRE(s1[l] && t1[l] && w1s_f16[l] && w3s_f16[l], "tn_dbg_dense_strip_pair_chain_dev: null operand");
    tab[l] = DenseStripLayerDev{s1[l], t1[l], (const f16 *)w1s_f16[l], (const f16 *)w3s_f16[l]};
  }
  DenseStripLayerDev *dev = nullptr;
  TN_HIP_CHECK(hipMalloc((void **)&dev, sizeof(DenseStripLayerDev) * nl));
  int rc = TN_OK;
  if (hipMemcpy(dev, tab.data(), sizeof(DenseStripLayerDev) * nl, hipMemcpyHostToDevice) != hipSuccess) {
    tn_set_error("tn_dbg_dense_strip_pair_chain_dev: upload failed");
    rc = TN_ERR_HIP;
  }
  if (rc == TN_OK) {
    const DenseStripChainArgs c{(f16 *)buf_f16, ldc, K0, nl, dev, B, H, W};
    rc = launch_dense_strip_pair_chain(c, ctx->stream);
  }
  const hipError_t he = hipStreamSynchronize(ctx->stream);
  (void)hipFree(dev);
  if (rc == TN_OK && he != hipSuccess) {
    tn_set_error("tn_dbg_dense_strip_pair_chain_dev: the launch failed");
    rc = TN_ERR_HIP;
  }
  return rc;
}


// ---- the LDS-resident 7x7 dense block (dense_block7.hip) ----
// nl layers from K0 input channels: w1_all = the (128, K_l) 1x1 weights one after the other, s1_all / t1_all the folded BN1
// scale / shift (K_l each), s2_all / t2_all the folded BN2 scale / shift (128 per layer), w3_all nl x (32,128,3,3).
struct tn_dbg_block7 {
  tn_ctx *ctx;
  void *wa = nullptr, *wb = nullptr, *tab = nullptr;
  DenseBlock7Args args;
};

extern "C" int tn_dbg_block7_create(tn_ctx *ctx, int K0, int nl, const float *w1_all, const float *s1_all, const float *t1_all,
                                    const float *s2_all, const float *t2_all, const float *w3_all, void **out) {
  TN_REQUIRE(ctx && w1_all && s1_all && t1_all && s2_all && t2_all && w3_all && out, "tn_dbg_block7_create: null argument");
  TN_REQUIRE(dense_block7_supported(7, 7, K0, nl), std::string("tn_dbg_block7_create: unsupported geometry (dense_block7 runs ") + kDenseBlock7Range + "): 7 x 7, K0 = " + std::to_string(K0) +
                                                       ", nl = " + std::to_string(nl));
  TN_ON_DEVICE(ctx->device);
  std::vector<std::vector<float>> folded(nl);
  std::vector<Block7Layer> layers(nl);
  size_t o1 = 0, ok = 0;
  for (int l = 0; l < nl; ++l) {
    const int K = K0 + 32 * l;
    folded[l].resize((size_t)128 * K);
    for (int n = 0; n < 128; ++n)
      for (int k = 0; k < K; ++k) folded[l][(size_t)n * K + k] = w1_all[o1 + (size_t)n * K + k] * s2_all[(size_t)l * 128 + n];
    layers[l] = Block7Layer{folded[l].data(), w3_all + (size_t)l * 32 * 128 * 9, s1_all + ok, t1_all + ok, t2_all + (size_t)l * 128};
    o1 += (size_t)128 * K;
    ok += K;
  }
  const Block7Image img = pack_block7(layers, K0);
  tn_dbg_block7 *b = new tn_dbg_block7();
  b->ctx = ctx;
  auto up = [&](void **dst, const void *src, size_t bytes) {
    if (hipMalloc(dst, bytes) != hipSuccess) return false;
    return hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  if (!up(&b->wa, img.wa.data(), img.wa.size() * sizeof(f16)) || !up(&b->wb, img.wb.data(), img.wb.size() * sizeof(f16)) ||
      !up(&b->tab, img.tab.data(), img.tab.size() * sizeof(float))) {
    tn_set_error("tn_dbg_block7_create: device allocation failed");
    return TN_ERR_NOMEM;
  }
  b->args = DenseBlock7Args{nullptr, 0, K0, nl, 0, (const f16 *)b->wa, (const f16 *)b->wb, (const float *)b->tab};
  for (int w = 0; w < 4; ++w) { b->args.a_off[w] = img.a_off[w]; b->args.b_off[w] = img.b_off[w]; }
  *out = b;
  return TN_OK;
}

extern "C" int tn_dbg_block7_run_ts(void *handle, void *buf_f16, int ldc, int B, unsigned long long *ts);
extern "C" int tn_dbg_block7_run(void *handle, void *buf_f16, int ldc, int B) { return tn_dbg_block7_run_ts(handle, buf_f16, ldc, B, nullptr); }
extern "C" int tn_dbg_block7_run_ts(void *handle, void *buf_f16, int ldc, int B, unsigned long long *ts) {
  tn_dbg_block7 *b = (tn_dbg_block7 *)handle;
  TN_REQUIRE(b && buf_f16, "tn_dbg_block7_run: null argument");
  TN_ON_DEVICE(b->ctx->device);
  DenseBlock7Args a = b->args;
  a.buf = (f16 *)buf_f16; a.ldc = ldc; a.B = B; a.ts = ts;
  return launch_dense_block7(a, b->ctx->stream);
}

// tn_dbg_block7_run with the fp32 side copy (side: device fp32 [B][49][ldc], or NULL) or with the head folded into the append (round
// 10; feat: device fp32 with row pitch ldfeat, head_s / head_t: device fp32 indexed by the concat buffer's channel; or all NULL).
// ts as tn_dbg_block7_run_ts.  Asynchronous.
extern "C" int tn_dbg_block7_run_head(void *handle, void *buf_f16, int ldc, int B, float *side, float *feat, const float *head_s,
                                      const float *head_t, int ldfeat, unsigned long long *ts) {
  tn_dbg_block7 *b = (tn_dbg_block7 *)handle;
  TN_REQUIRE(b && buf_f16, "tn_dbg_block7_run_head: null argument");
  TN_REQUIRE(((uintptr_t)side & 15) == 0, "tn_dbg_block7_run_head: side must be 16-byte aligned");
  TN_ON_DEVICE(b->ctx->device);
  DenseBlock7Args a = b->args;
  a.buf = (f16 *)buf_f16; a.ldc = ldc; a.B = B; a.ts = ts;
  a.side = side;
  a.feat = feat; a.head_s = head_s; a.head_t = head_t; a.ldfeat = ldfeat;
  return launch_dense_block7(a, b->ctx->stream);
}

extern "C" void tn_dbg_block7_destroy(void *handle) {
  tn_dbg_block7 *b = (tn_dbg_block7 *)handle;
  if (!b) return;
  (void)hipFree(b->wa); (void)hipFree(b->wb); (void)hipFree(b->tab);
  delete b;
}


// ---- the streamed dense blocks (dense_block14.hip, dense_block28.hip): one implementation behind both sets of symbols ----
// same operand convention as tn_dbg_block7_create
struct tn_dbg_stream_block {
  tn_ctx *ctx;
  const DenseStreamKernel *kernel;
  void *stream = nullptr, *scratch = nullptr;
  int scratch_frames = 0;
  DenseStreamArgs args;
};

// (a handle is served by the kernel that created it, whichever of the run / destroy symbols it is passed to)
static_assert(sizeof(kDenseStreamKernels) / sizeof(kDenseStreamKernels[0]) == 2 && kDenseStreamKernels[0].H == 14 && kDenseStreamKernels[1].H == 28,
              "tn_dbg_block14_* / tn_dbg_block28_* index the table");
static int dbg_stream_create(const DenseStreamKernel &sk, tn_ctx *ctx, int K0, int nl, const float *w1_all, const float *s1_all, const float *t1_all,
                             const float *s2_all, const float *t2_all, const float *w3_all, void **out) {
  const std::string who = "tn_dbg_block" + std::to_string(sk.H) + "_create";
  TN_REQUIRE(ctx && w1_all && s1_all && t1_all && s2_all && t2_all && w3_all && out, who + ": null argument");
  TN_REQUIRE(sk.supported(sk.H, sk.H, K0, nl), who + ": unsupported geometry (dense_block" + std::to_string(sk.H) + " runs " + sk.range + "): " + std::to_string(sk.H) + " x " + std::to_string(sk.H) +
                                                   ", K0 = " + std::to_string(K0) + ", nl = " + std::to_string(nl));
  TN_ON_DEVICE(ctx->device);
  std::vector<std::vector<float>> folded(nl);
  std::vector<Block14Layer> layers(nl);
  size_t o1 = 0, ok = 0;
  for (int l = 0; l < nl; ++l) {
    const int K = K0 + 32 * l;
    folded[l].resize((size_t)128 * K);
    for (int n = 0; n < 128; ++n)
      for (int k = 0; k < K; ++k) folded[l][(size_t)n * K + k] = w1_all[o1 + (size_t)n * K + k] * s2_all[(size_t)l * 128 + n];
    layers[l] = Block14Layer{folded[l].data(), w3_all + (size_t)l * 32 * 128 * 9, s1_all + ok, t1_all + ok, t2_all + (size_t)l * 128};
    o1 += (size_t)128 * K;
    ok += K;
  }
  const std::vector<unsigned char> img = sk.pack(layers, K0);
  tn_dbg_stream_block *b = new tn_dbg_stream_block();
  b->ctx = ctx;
  b->kernel = &sk;
  if (hipMalloc(&b->stream, img.size()) != hipSuccess || hipMemcpy(b->stream, img.data(), img.size(), hipMemcpyHostToDevice) != hipSuccess) {
    tn_set_error(who + ": device allocation failed");
    delete b;
    return TN_ERR_NOMEM;
  }
  b->args = DenseStreamArgs{nullptr, 0, K0, nl, 0, (const unsigned char *)b->stream, sk.units(K0, nl)};
  *out = b;
  return TN_OK;
}

static int dbg_stream_run(void *handle, void *buf_f16, int ldc, int B, unsigned long long *ts) {
  tn_dbg_stream_block *b = (tn_dbg_stream_block *)handle;
  TN_REQUIRE(b && buf_f16, "tn_dbg_block14_run / tn_dbg_block28_run: null argument");
  const std::string who = "tn_dbg_block" + std::to_string(b->kernel->H) + "_run";
  TN_REQUIRE(B > 0, who + ": the batch must be positive: " + std::to_string(b->kernel->H) + " x " + std::to_string(b->kernel->H) + ", K0 = " + std::to_string(b->args.K0) +
                        ", nl = " + std::to_string(b->args.nl) + ", ldc = " + std::to_string(ldc) + ", B = " + std::to_string(B));
  TN_ON_DEVICE(b->ctx->device);
  const size_t scratch_bytes = (size_t)B * b->kernel->scratch_halfs() * sizeof(f16);
  if (b->scratch_frames < B) {
    (void)hipFree(b->scratch);
    b->scratch = nullptr; b->scratch_frames = 0;
    if (hipMalloc(&b->scratch, scratch_bytes) != hipSuccess) {
      tn_set_error(who + ": device allocation failed");
      return TN_ERR_NOMEM;
    }
    b->scratch_frames = B;
    TN_HIP_CHECK(hipMemset(b->scratch, 0, scratch_bytes));
  }
  DenseStreamArgs a = b->args;
  a.buf = (f16 *)buf_f16; a.ldc = ldc; a.B = B; a.ts = ts; a.scratch = (f16 *)b->scratch;
  return b->kernel->launch(a, b->ctx->stream);
}

static void dbg_stream_destroy(void *handle) {
  tn_dbg_stream_block *b = (tn_dbg_stream_block *)handle;
  if (!b) return;
  (void)hipFree(b->stream);
  (void)hipFree(b->scratch);
  delete b;
}

extern "C" int tn_dbg_block14_create(tn_ctx *ctx, int K0, int nl, const float *w1_all, const float *s1_all, const float *t1_all,
                                     const float *s2_all, const float *t2_all, const float *w3_all, void **out) {
  return dbg_stream_create(kDenseStreamKernels[0], ctx, K0, nl, w1_all, s1_all, t1_all, s2_all, t2_all, w3_all, out);
}
extern "C" int tn_dbg_block14_run_ts(void *handle, void *buf_f16, int ldc, int B, unsigned long long *ts) { return dbg_stream_run(handle, buf_f16, ldc, B, ts); }
extern "C" int tn_dbg_block14_run(void *handle, void *buf_f16, int ldc, int B) { return dbg_stream_run(handle, buf_f16, ldc, B, nullptr); }
extern "C" void tn_dbg_block14_destroy(void *handle) { dbg_stream_destroy(handle); }

extern "C" int tn_dbg_block28_create(tn_ctx *ctx, int K0, int nl, const float *w1_all, const float *s1_all, const float *t1_all,
                                     const float *s2_all, const float *t2_all, const float *w3_all, void **out) {
  return dbg_stream_create(kDenseStreamKernels[1], ctx, K0, nl, w1_all, s1_all, t1_all, s2_all, t2_all, w3_all, out);
}
extern "C" int tn_dbg_block28_run_ts(void *handle, void *buf_f16, int ldc, int B, unsigned long long *ts) { return dbg_stream_run(handle, buf_f16, ldc, B, ts); }
extern "C" int tn_dbg_block28_run(void *handle, void *buf_f16, int ldc, int B) { return dbg_stream_run(handle, buf_f16, ldc, B, nullptr); }
extern "C" void tn_dbg_block28_destroy(void *handle) { dbg_stream_destroy(handle); }

// The fine-tuning step's transposed GEMM (weight gradients): the split-K policy of gemm_tn_dispatch on the caller's workspace
extern "C" int tn_dbg_gemm_tn(tn_ctx *ctx, const float *A, int lda, const float *B, int ldb, const float *bsc, const float *bsh, float *Cm,
                              int ldc, int M, int N, int K, float *workspace, int64_t workspace_floats) {
  TN_REQUIRE(ctx && A && B && Cm && (bsc == nullptr) == (bsh == nullptr), "tn_dbg_gemm_tn: null argument");
  TN_REQUIRE(M > 0 && N > 0 && K > 0 && lda >= M && ldb >= N && ldc >= N && workspace_floats >= 0, "tn_dbg_gemm_tn: bad shape");
  TN_ON_DEVICE(ctx->device);
  const int rc = bsc ? launch_gemm_tn_f32_bnrelu(A, lda, B, ldb, bsc, bsh, Cm, ldc, M, N, K, ctx->stream, workspace, workspace_floats)
                     : launch_gemm_tn_f32(A, lda, B, ldb, Cm, ldc, M, N, K, ctx->stream, workspace, workspace_floats);
  if (rc) return rc;
  TN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return TN_OK;
}

// The NN-layout product of the CNN-RNN step (dX = dGI W_ih), through the step's launcher
extern "C" int tn_dbg_gemm_nn(tn_ctx *ctx, const float *A, int lda, const float *B, int ldb, float *Cm, int ldc, int M, int N, int K) {
  TN_REQUIRE(ctx && A && B && Cm, "tn_dbg_gemm_nn: null argument");
  TN_REQUIRE(M > 0 && N > 0 && K > 0 && lda >= K && ldb >= N && ldc >= N, "tn_dbg_gemm_nn: bad shape");
  TN_ON_DEVICE(ctx->device);
  const int rc = launch_gemm_nn_f32(A, lda, B, ldb, Cm, ldc, M, N, K, 0, ctx->stream);
  if (rc) return rc;
  TN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return TN_OK;
}

// The clipping reduction of the training steps (train.hip launch_grad_sumsq) on caller buffers; max_norm 0: no scale, no count
extern "C" int tn_dbg_grad_sumsq(tn_ctx *ctx, const float *dev, int64_t n, const float *dev2, int64_t n2, double *sumsq_host) {
  TN_REQUIRE(ctx && sumsq_host, "tn_dbg_grad_sumsq: null argument");
  TN_REQUIRE(n >= 0 && n2 >= 0 && (dev || !n) && (dev2 || !n2), "tn_dbg_grad_sumsq: a non-empty segment needs a pointer, counts >= 0");
  TN_ON_DEVICE(ctx->device);
  void *ws = nullptr;
  const size_t part_bytes = sizeof(float) * TN_GRAD_SUMSQ_GRID;
  TN_HIP_CHECK(hipMalloc(&ws, part_bytes + sizeof(tn_clip_record)));
  tn_clip_record *rec = (tn_clip_record *)((char *)ws + part_bytes), r;
  int rc = launch_grad_sumsq(dev, n, dev2, n2, 1.f, 0.f, (float *)ws, rec, ctx->stream);
  hipError_t e = hipSuccess;
  if (!rc) e = hipMemcpyAsync(&r, rec, sizeof(r), hipMemcpyDeviceToHost, ctx->stream);
  if (!rc && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(ws);
  if (rc) return rc;
  TN_HIP_CHECK(e);
  *sumsq_host = r.sumsq;
  return TN_OK;
}

// The recurrent kernels' dispatch policy (rnn.h rnn_route: what launch_rnn_recurrent and rnn_bptt.hip's launch_rnn_bptt both follow) for a
// shape; host arithmetic only, no device is touched
extern "C" int tn_dbg_rnn_route(int gates, int B, int H, int dirs, int *nb, int *kr, int *big) {
  TN_REQUIRE(nb && kr && big, "tn_dbg_rnn_route: null argument");
  TN_REQUIRE(gates == 3 || gates == 4, "tn_dbg_rnn_route: gates must be 3 or 4");
  TN_REQUIRE(B > 0 && (dirs == 1 || dirs == 2) && H > 0 && gates * H <= 1024 && H % 4 == 0,
             "tn_dbg_rnn_route: gates*hidden must be <= 1024, hidden % 4 == 0, batch > 0, dirs 1 or 2");
  const tn_rnn_route r = rnn_route(gates, B, H, dirs);
  *nb = r.nb; *kr = r.kr; *big = r.big;
  return TN_OK;
}

// The wide recurrent kernels' dispatch policy (rnn.h rnn_wide_route) for the shapes that need it, 1024 < gates*H <= 2048; host arithmetic
// only, no device is touched
extern "C" int tn_dbg_rnn_wide_route(int gates, int B, int H, int dirs, int *threads, int *rows, int *nb, int64_t *lds_fwd, int64_t *lds_bwd) {
  TN_REQUIRE(threads && rows && nb && lds_fwd && lds_bwd, "tn_dbg_rnn_wide_route: null argument");
  TN_REQUIRE(gates == 3 || gates == 4, "tn_dbg_rnn_wide_route: gates must be 3 or 4");
  TN_REQUIRE(B > 0 && (dirs == 1 || dirs == 2) && H > 0 && gates * H > 1024 && gates * H <= 2048 && H % 4 == 0,
             "tn_dbg_rnn_wide_route: gates*hidden must be in (1024, 2048], hidden % 4 == 0, batch > 0, dirs 1 or 2");
  const tn_rnn_wide_route r = rnn_wide_route(gates, B, H, dirs);
  *threads = r.threads; *rows = r.rows; *nb = r.nb; *lds_fwd = (int64_t)r.lds_fwd; *lds_bwd = (int64_t)r.lds_bwd;
  return TN_OK;
}

// Test hook: every recurrent launch of the process takes the wide kernels, the shapes the one-row-per-thread kernels serve included
extern "C" int tn_dbg_rnn_force_wide(int on) {
  rnn_set_force_wide(on != 0);
  return TN_OK;
}

extern "C" int tn_dbg_rnn_wide_launches(int64_t *count) {
  TN_REQUIRE(count, "tn_dbg_rnn_wide_launches: null argument");
  *count = (int64_t)rnn_wide_launches();
  return TN_OK;
}

// The parameter table of a training handle, from the builder its create calls (param_table.h); host arithmetic only, no device
extern "C" int tn_dbg_trainer_params(int which, const int *dims, int n_dims, const char *prefix_a, const char *prefix_b, tn_param_row *rows,
                                     int max_rows, int *n_rows, int64_t *numel, int64_t *state_numel) {
  TN_REQUIRE(dims && prefix_a && n_rows && (rows || max_rows == 0), "tn_dbg_trainer_params: null argument");
  ParamTable t;
  if (which == TN_TRAINER_HEAD) {
    TN_REQUIRE(n_dims == 4 && prefix_b, "tn_dbg_trainer_params: the head takes (gates, input, hidden, classes) and two prefixes");
    HeadOffsets o;
    t = head_param_table(dims[0], dims[1], dims[2], dims[3], prefix_a, prefix_b, &o);
  } else if (which == TN_TRAINER_GNMT) {
    TN_REQUIRE(n_dims == 7 && dims[5] >= 2 && dims[6] >= 0 && dims[6] < dims[5],
               "tn_dbg_trainer_params: the captioner takes (gates, input, hidden, embed, vocab, num_layers, num_bi_layers < num_layers)");
    GnmtOffsets o;
    t = gnmt_param_table(dims[0], dims[1], dims[2], dims[3], dims[4], dims[5], dims[6], prefix_a, &o);
  } else if (which == TN_TRAINER_BACKBONE) {
    TN_REQUIRE(n_dims == 1 && (dims[0] > 0) == (prefix_b != nullptr),
               "tn_dbg_trainer_params: the backbone takes (classes) and the classifier's prefix, or (0) and none");
    FtNet net;
    t = ft_param_table(prefix_a, prefix_b, dims[0], &net);
  } else {
    TN_REQUIRE(false, "tn_dbg_trainer_params: which must be TN_TRAINER_HEAD, TN_TRAINER_GNMT or TN_TRAINER_BACKBONE");
  }
  for (size_t i = 0; i < t.rows.size() && (int)i < max_rows; ++i) {
    const ParamTable::Row &r = t.rows[i];
    TN_REQUIRE(r.name.size() < sizeof(rows[i].name), "tn_dbg_trainer_params: a name does not fit tn_param_row");
    memset(&rows[i], 0, sizeof(rows[i]));
    memcpy(rows[i].name, r.name.data(), r.name.size());
    rows[i].where = (int)r.where; rows[i].offset = r.off; rows[i].count = r.count;
  }
  *n_rows = (int)t.rows.size();
  if (numel) *numel = t.n;
  if (state_numel) *state_numel = t.ns;
  return TN_OK;
}

// The fp16 encoder's launches for an input size, create flags (and the TN_* environment of the call), batch and pass, as
// tn_densenet121_profile would report them: families in first-seen order with launches, flops and bytes (ms 0).  Built from
// what create and encoder_run_range follow (encoder_plan.h: enc_policy, enc_geom, enc_block_plan); host arithmetic only, no device
// is touched.  Refuses what create refuses for the size and the flags, and the fp32 / fp32x3 modes, which are not planned.
static int encoder_plan_stats(int height, int width, int flags, int batch, int calibrate, bool shared_chip, tn_kernel_stat *stats, int max_stats,
                              int *n_stats, int *paired_out) {
  TN_REQUIRE(stats && n_stats && max_stats > 0, "tn_dbg_encoder_plan: null argument");
  TN_REQUIRE((flags & ~TN_ENC_EXACT_WEIGHTS) == 0, "tn_dbg_encoder_plan: unknown flag, or a mode that is not planned (TN_ENC_FP32, TN_ENC_FP32X3)");
  TN_REQUIRE(batch > 0, "tn_dbg_encoder_plan: batch must be positive");
  TN_REQUIRE(height >= 224 && width >= 224 && height <= 1024 && width <= 1024, "tn_dbg_encoder_plan: input size must be in [224,1024]");
  const EncPolicy p = enc_policy(flags);
  const EncGeom g = enc_geom(height, width);
  if (const char *why = enc_refusal(p, g)) { tn_set_error(why); return TN_ERR_INVALID; }
  std::vector<tn_kernel_stat> fams;
  auto add = [&](const std::string &name, const EncCost &c) {
    size_t i = 0;
    while (i < fams.size() && name != fams[i].name) ++i;
    if (i == fams.size()) {
      tn_kernel_stat st;
      memset(&st, 0, sizeof(st));
      strncpy(st.name, name.c_str(), sizeof(st.name) - 1);
      fams.push_back(st);
    }
    fams[i].launches += 1;
    fams[i].flops += c.flops;
    fams[i].bytes += c.bytes;
  };
  const double fB = (double)batch;
  int paired = 0;
  if (p.fuse) {
    add("stem_conv_bn_relu_maxpool", stem_pool_cost(g, fB));
  } else {
    add("stem_conv7x7_bn_relu", stem_cost(g, fB));
    add("maxpool3x3s2", maxpool_cost(g, fB));
  }
  for (int b = 0; b < 4; ++b) {
    const int M = batch * g.Hb[b] * g.Wb[b];
    for (const EncStep &st : enc_block_plan(p, g, b, batch, calibrate != 0, shared_chip)) {
      if (st.paired) ++paired;
      if (st.route == ENC_LAYERWISE) {
        add(family_name(st, g, b), conv1x1_cost(M, enc_layer_cin(g, b, st.l0)));
        add("conv3x3_bnrelu", conv3x3_cost(M));
      } else {
        add(family_name(st, g, b), step_cost(st, g, b, M));
      }
    }
    if (b < 3) add("transition_conv1x1_avgpool", transition_cost(M, batch * g.Hb[b + 1] * g.Wb[b + 1], g.Cb[b], g.Cb[b] / 2));
  }
  add("head_bnrelu_avgpool7", head_cost(g, fB));
  const int n = (int)fams.size() < max_stats ? (int)fams.size() : max_stats;
  for (int i = 0; i < n; ++i) stats[i] = fams[i];
  *n_stats = n;
  if (paired_out) *paired_out = paired;
  return TN_OK;
}

extern "C" int tn_dbg_encoder_plan(int height, int width, int flags, int batch, int calibrate, tn_kernel_stat *stats, int max_stats,
                                   int *n_stats) {
  return encoder_plan_stats(height, width, flags, batch, calibrate, false, stats, max_stats, n_stats, nullptr);
}

// The plan of a forward whose kernels share the chip with a neighbouring stream's call (the interleaved whole-batch branch of
// encoder_run; never the calibration pass): the same families, launches, flops and bytes, and *paired_out: how many of its steps take
// the paired launch geometry of the 28x28 strip kernels (encoder_plan.h::enc_strip_pair)
extern "C" int tn_dbg_encoder_plan_shared(int height, int width, int flags, int batch, tn_kernel_stat *stats, int max_stats, int *n_stats,
                                          int *paired_out) {
  TN_REQUIRE(paired_out, "tn_dbg_encoder_plan_shared: null argument");
  return encoder_plan_stats(height, width, flags, batch, 0, true, stats, max_stats, n_stats, paired_out);
}

extern "C" int tn_dbg_strip_pair_launches(int64_t *count) {
  TN_REQUIRE(count, "tn_dbg_strip_pair_launches: null argument");
  *count = (int64_t)strip_pair_launches();
  return TN_OK;
}

// launches with the head folded in so far in this process: one per frame range from the last transition, one from the 7x7 block
extern "C" int tn_dbg_head_fused_launches(int64_t *count) {
  TN_REQUIRE(count, "tn_dbg_head_fused_launches: null argument");
  *count = (int64_t)head_fused_launches();
  return TN_OK;
}

// encoder_plan.h::enc_head_fused for an input size, create flags (and the TN_* environment of the call), batch, pass and entry point:
// *fused = 1 where a forward takes the route, 0 where it keeps the side copy and the head launch (the fp32 / fp32x3 modes: always 0).
// Host arithmetic only; the instrumented pass never takes the route and is not asked about.
extern "C" int tn_dbg_head_fused(int height, int width, int flags, int batch, int calibrate, int class_maps, int *fused) {
  TN_REQUIRE(fused, "tn_dbg_head_fused: null argument");
  TN_REQUIRE((flags & ~(TN_ENC_EXACT_WEIGHTS | TN_ENC_FP32 | TN_ENC_FP32X3)) == 0, "tn_dbg_head_fused: unknown flag");
  TN_REQUIRE(batch > 0, "tn_dbg_head_fused: batch must be positive");
  TN_REQUIRE(height >= 224 && width >= 224 && height <= 1024 && width <= 1024, "tn_dbg_head_fused: input size must be in [224,1024]");
  const EncPolicy p = enc_policy(flags);
  const EncGeom g = enc_geom(height, width);
  if (const char *why = enc_refusal(p, g)) { tn_set_error(why); return TN_ERR_INVALID; }
  const bool fp32 = (flags & (TN_ENC_FP32 | TN_ENC_FP32X3)) != 0;
  *fused = !fp32 && enc_head_fused(p, g, calibrate != 0, class_maps != 0, false) ? 1 : 0;
  return TN_OK;
}

// The captioner's training step with its source gradient (train.h::gnmt_trainer_step), what the frame-mode step hands to the backbone
extern "C" int tn_dbg_gnmt_trainer_src_grad(tn_gnmt_trainer *t, const float *src, const int32_t *src_valid_len, const int32_t *tgt, int ld,
                                            const int32_t *tgt_valid_len, int batch, int steps, int tgt_len, float *loss,
                                            float *logits_out, float *dsrc, int ldd) {
  TN_REQUIRE(t && dsrc, "tn_dbg_gnmt_trainer_src_grad: null argument");
  return gnmt_trainer_step(t, src, src_valid_len, tgt, ld, tgt_valid_len, batch, steps, tgt_len, loss, logits_out, dsrc, ldd);
}

// Measurement switch of the pad-row gathered linear kernels (linear.h): 0 launches the instantiation without the pad-tile skip
extern "C" int tn_dbg_rows_pad_skip(int on) {
  linear_rows_set_pad_skip(on != 0);
  return TN_OK;
}

// The forward 1x1 convolution of the fine-tuning step with its BatchNorm + ReLU applied to the X operand
extern "C" int tn_dbg_linear_bnrelu(tn_ctx *ctx, const float *X, int ldx, const float *asc, const float *ash, const float *W, int ldw,
                                    const float *bias, float *Y, int ldy, int M, int N, int K, int accumulate) {
  TN_REQUIRE(ctx && X && asc && ash && W && Y, "tn_dbg_linear_bnrelu: null argument");
  TN_REQUIRE(M > 0 && N > 0 && K > 0 && ldx >= K && ldw >= K && ldy >= N, "tn_dbg_linear_bnrelu: bad shape");
  TN_ON_DEVICE(ctx->device);
  const int rc = launch_linear_f32_bnrelu(X, ldx, asc, ash, W, ldw, bias, Y, ldy, M, N, K, accumulate, ctx->stream);
  if (rc) return rc;
  TN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return TN_OK;
}

// The fp32x3 twins of the two hooks above (gemm_fp32x3.hip), through the launchers the step calls in TN_MATMUL_FP32X3
extern "C" int tn_dbg_linear_fp32x3(tn_ctx *ctx, const float *X, int ldx, const float *asc, const float *ash, const float *W, int ldw,
                                    const float *bias, float *Y, int ldy, int M, int N, int K, int accumulate) {
  TN_REQUIRE(ctx && X && W && Y && (asc == nullptr) == (ash == nullptr), "tn_dbg_linear_fp32x3: null argument");
  TN_REQUIRE(M > 0 && N > 0 && K > 0 && ldx >= K && ldw >= K && ldy >= N, "tn_dbg_linear_fp32x3: bad shape");
  TN_ON_DEVICE(ctx->device);
  const int rc = launch_linear_fp32x3(X, ldx, asc, ash, W, ldw, bias, Y, ldy, M, N, K, accumulate, ctx->stream);
  if (rc) return rc;
  TN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return TN_OK;
}
extern "C" int tn_dbg_gemm_tn_fp32x3(tn_ctx *ctx, const float *A, int lda, const float *B, int ldb, const float *bsc, const float *bsh,
                                     float *Cm, int ldc, int M, int N, int K, float *workspace, int64_t workspace_floats) {
  TN_REQUIRE(ctx && A && B && Cm && (bsc == nullptr) == (bsh == nullptr), "tn_dbg_gemm_tn_fp32x3: null argument");
  TN_REQUIRE(M > 0 && N > 0 && K > 0 && lda >= M && ldb >= N && ldc >= N && workspace_floats >= 0, "tn_dbg_gemm_tn_fp32x3: bad shape");
  TN_ON_DEVICE(ctx->device);
  const int rc = launch_gemm_tn_fp32x3(A, lda, B, ldb, bsc, bsh, Cm, ldc, M, N, K, ctx->stream, workspace, workspace_floats);
  if (rc) return rc;
  TN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return TN_OK;
}

// The fine-tuning step's training-mode BatchNorm + ReLU and its backward (the same reduction slices as the step), scratch of its own
extern "C" int tn_dbg_bn_train(tn_ctx *ctx, const float *x, int ld, int64_t M, int C, const float *gamma, const float *beta, float *mean,
                               float *var, float *y, const float *dy, float *dgamma, float *dbeta, float *dx, int ldd, int accumulate) {
  TN_REQUIRE(ctx && x && gamma && beta && mean && var && y, "tn_dbg_bn_train: null argument");
  TN_REQUIRE(!dy || (dgamma && dbeta && dx), "tn_dbg_bn_train: dy needs dgamma, dbeta and dx");
  TN_REQUIRE(M > 0 && C > 0 && ld >= C && (!dy || ldd >= C), "tn_dbg_bn_train: bad shape");
  TN_ON_DEVICE(ctx->device);
  float *ws = nullptr;
  TN_HIP_CHECK(hipMalloc((void **)&ws, sizeof(float) * ft_bn_ws_floats((long)M, C)));
  int rc = launch_ft_bn_stats(x, ld, (long)M, C, ws, mean, var, ctx->stream);
  if (!rc) rc = launch_ft_bn_relu(x, ld, (long)M, C, mean, var, gamma, beta, y, ctx->stream);
  if (!rc && dy) rc = launch_ft_bn_backward(dy, x, ld, (long)M, C, mean, var, gamma, beta, ws, dgamma, dbeta, dx, ldd, accumulate, ctx->stream);
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(ws);
  if (rc) return rc;
  TN_HIP_CHECK(e);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

// ---- the training steps' operator kernels, alone (finetune.hip launch_ft_*, train.hip) ----
// Each hook checks what its kernel cannot take, runs the operator through the launcher the step calls on the context's stream and
// synchronises.  Nothing is launched after a refusal.
namespace {
inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline bool fits_int(long n) { return n > 0 && n <= 0x7fffffffL; }
int dbg_finish(tn_ctx *ctx, int rc) {
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (rc) return rc;
  TN_HIP_CHECK(e);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}
}  // namespace

extern "C" int tn_dbg_ft_im2col7(tn_ctx *ctx, const float *x, int B, int H, int W, float *col) {
  TN_REQUIRE(ctx && x && col, "tn_dbg_ft_im2col7: null argument");
  TN_REQUIRE(B > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "tn_dbg_ft_im2col7: B, H, W must be positive, H and W even");
  TN_ON_DEVICE(ctx->device);
  return dbg_finish(ctx, launch_ft_im2col7(x, B, H, W, col, ctx->stream));
}
extern "C" int tn_dbg_ft_im2col3(tn_ctx *ctx, const float *a, int B, int H, int W, int C, const float *sc, const float *sh, float *col) {
  TN_REQUIRE(ctx && a && col && (sc == nullptr) == (sh == nullptr), "tn_dbg_ft_im2col3: null argument (sc and sh go together)");
  TN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "tn_dbg_ft_im2col3: B, H, W, C must be positive, C a multiple of 4");
  TN_REQUIRE(al16(a) && al16(col) && al16(sc) && al16(sh), "tn_dbg_ft_im2col3: the buffers must be 16-byte aligned");
  TN_ON_DEVICE(ctx->device);
  return dbg_finish(ctx, launch_ft_im2col3(a, B, H, W, C, col, sc, sh, ctx->stream));
}
extern "C" int tn_dbg_ft_col2im3(tn_ctx *ctx, const float *dcol, int B, int H, int W, int C, float *da) {
  TN_REQUIRE(ctx && dcol && da, "tn_dbg_ft_col2im3: null argument");
  TN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "tn_dbg_ft_col2im3: B, H, W, C must be positive, C a multiple of 4");
  TN_REQUIRE(al16(dcol) && al16(da), "tn_dbg_ft_col2im3: the buffers must be 16-byte aligned");
  TN_ON_DEVICE(ctx->device);
  return dbg_finish(ctx, launch_ft_col2im3(dcol, B, H, W, C, da, ctx->stream));
}
// y non-null: the forward; dy and da non-null (together): the gradient.  At least one of the two.
extern "C" int tn_dbg_ft_maxpool(tn_ctx *ctx, const float *a, int B, int H, int W, int C, float *y, int ldy, const float *dy, float *da) {
  TN_REQUIRE(ctx && a && (y || dy) && (dy == nullptr) == (da == nullptr), "tn_dbg_ft_maxpool: null argument (dy and da go together)");
  TN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0, "tn_dbg_ft_maxpool: B, H, W, C must be positive, H and W even");
  TN_REQUIRE(ldy >= C, "tn_dbg_ft_maxpool: ldy below C");
  TN_ON_DEVICE(ctx->device);
  int rc = y ? launch_ft_maxpool(a, B, H, W, C, y, ldy, ctx->stream) : TN_OK;
  if (!rc && dy) rc = launch_ft_maxpool_bwd(a, dy, ldy, B, H, W, C, da, ctx->stream);
  return dbg_finish(ctx, rc);
}
// z and y non-null (together): the forward; dy and dz non-null (together): the gradient.  At least one of the two.
extern "C" int tn_dbg_ft_avgpool2(tn_ctx *ctx, const float *z, int B, int H, int W, int C, float *y, int ldy, const float *dy, float *dz) {
  TN_REQUIRE(ctx && (z || dy) && (z == nullptr) == (y == nullptr) && (dy == nullptr) == (dz == nullptr),
             "tn_dbg_ft_avgpool2: null argument (z with y, dy with dz)");
  TN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0, "tn_dbg_ft_avgpool2: B, H, W, C must be positive, H and W even");
  TN_REQUIRE(ldy >= C, "tn_dbg_ft_avgpool2: ldy below C");
  TN_ON_DEVICE(ctx->device);
  int rc = z ? launch_ft_avgpool2(z, B, H, W, C, y, ldy, ctx->stream) : TN_OK;
  if (!rc && dy) rc = launch_ft_avgpool2_bwd(dy, ldy, B, H, W, C, dz, ctx->stream);
  return dbg_finish(ctx, rc);
}
// a and f non-null (together): the forward; df and da non-null (together): the gradient.  At least one of the two.
extern "C" int tn_dbg_ft_gap(tn_ctx *ctx, const float *a, int B, int P, int C, float *f, const float *df, float *da) {
  TN_REQUIRE(ctx && (a || df) && (a == nullptr) == (f == nullptr) && (df == nullptr) == (da == nullptr),
             "tn_dbg_ft_gap: null argument (a with f, df with da)");
  TN_REQUIRE(B > 0 && P > 0 && C > 0 && fits_int((long)B * C), "tn_dbg_ft_gap: B, P, C must be positive, B C below 2^31");
  TN_ON_DEVICE(ctx->device);
  int rc = a ? launch_ft_gap(a, B, P, C, f, ctx->stream) : TN_OK;
  if (!rc && df) rc = launch_ft_gap_bwd(df, B, P, C, da, ctx->stream);
  return dbg_finish(ctx, rc);
}
extern "C" int tn_dbg_ft_bn_fold(tn_ctx *ctx, const float *mean, const float *var, const float *gamma, const float *beta, int C, float *sc,
                                 float *sh) {
  TN_REQUIRE(ctx && mean && var && gamma && beta && sc && sh, "tn_dbg_ft_bn_fold: null argument");
  TN_REQUIRE(C > 0, "tn_dbg_ft_bn_fold: C must be positive");
  TN_ON_DEVICE(ctx->device);
  return dbg_finish(ctx, launch_ft_bn_fold(mean, var, gamma, beta, C, sc, sh, ctx->stream));
}
extern "C" int tn_dbg_ft_bn_running(tn_ctx *ctx, float *rmean, float *rvar, const float *mean, const float *var, int C) {
  TN_REQUIRE(ctx && rmean && rvar && mean && var, "tn_dbg_ft_bn_running: null argument");
  TN_REQUIRE(C > 0, "tn_dbg_ft_bn_running: C must be positive");
  TN_ON_DEVICE(ctx->device);
  return dbg_finish(ctx, launch_ft_bn_running(rmean, rvar, mean, var, C, ctx->stream));
}
// Max over time with the first argmax; dpooled and dseq non-null (together): then the scatter of dpooled through arg.
extern "C" int tn_dbg_pool_max_arg(tn_ctx *ctx, const float *x, int B, int T, int F, float *y, int32_t *arg, const float *dpooled, float *dseq) {
  TN_REQUIRE(ctx && x && y && arg && (dpooled == nullptr) == (dseq == nullptr), "tn_dbg_pool_max_arg: null argument (dpooled and dseq go together)");
  TN_REQUIRE(B > 0 && T > 0 && F > 0, "tn_dbg_pool_max_arg: B, T, F must be positive");
  TN_ON_DEVICE(ctx->device);
  int rc = launch_pool_max_arg(x, B, T, F, y, arg, ctx->stream);
  if (!rc && dpooled) rc = launch_scatter_pool_grad(dpooled, arg, B, T, F, dseq, ctx->stream);
  return dbg_finish(ctx, rc);
}
// labels_host: the host copy of the device labels; the kernel indexes a row by its label unchecked, so the hook checks the copy.
extern "C" int tn_dbg_softmax_ce(tn_ctx *ctx, const float *logits, const int32_t *labels, const int32_t *labels_host, int B, int C, float *loss,
                                 float *dlogits) {
  TN_REQUIRE(ctx && logits && labels && labels_host && loss && dlogits, "tn_dbg_softmax_ce: null argument");
  TN_REQUIRE(B > 0 && C > 0, "tn_dbg_softmax_ce: B and C must be positive");
  for (int b = 0; b < B; ++b) TN_REQUIRE(labels_host[b] >= 0 && labels_host[b] < C, "tn_dbg_softmax_ce: a label lies outside [0, C)");
  TN_ON_DEVICE(ctx->device);
  return dbg_finish(ctx, launch_softmax_ce(logits, labels, B, C, loss, dlogits, ctx->stream));
}
extern "C" int tn_dbg_dense_bwd(tn_ctx *ctx, const float *dlogits, const float *pooled, const float *wd, int B, int C, int K, float *dwd,
                                float *dbd, float *dpooled) {
  TN_REQUIRE(ctx && dlogits && pooled && wd && dwd && dbd && dpooled, "tn_dbg_dense_bwd: null argument");
  TN_REQUIRE(B > 0 && C > 0 && K > 0 && fits_int((long)C * K) && fits_int((long)B * K) && fits_int((long)B * C),
             "tn_dbg_dense_bwd: B, C, K must be positive, their pairwise products below 2^31");
  TN_ON_DEVICE(ctx->device);
  return dbg_finish(ctx, launch_dense_bwd(dlogits, pooled, wd, B, C, K, dwd, dbd, dpooled, ctx->stream));
}
extern "C" int tn_dbg_colsum(tn_ctx *ctx, const float *A, int lda, int rows, int cols, float *out) {
  TN_REQUIRE(ctx && A && out, "tn_dbg_colsum: null argument");
  TN_REQUIRE(rows > 0 && cols > 0, "tn_dbg_colsum: rows and cols must be positive");
  TN_REQUIRE(lda >= cols, "tn_dbg_colsum: lda below cols");
  TN_ON_DEVICE(ctx->device);
  return dbg_finish(ctx, launch_colsum_f32(A, lda, rows, cols, out, ctx->stream));
}
// scale: a device float, or NULL for the un-clipped instantiation
extern "C" int tn_dbg_sgd_momentum(tn_ctx *ctx, float *w, const float *g, float *mom, int64_t n, float lr, float momentum, float wd,
                                   float rescale, const float *scale) {
  TN_REQUIRE(ctx && w && g && mom, "tn_dbg_sgd_momentum: null argument");
  TN_REQUIRE(n > 0, "tn_dbg_sgd_momentum: n must be positive");
  TN_ON_DEVICE(ctx->device);
  return dbg_finish(ctx, launch_sgd_momentum(w, g, mom, (long)n, lr, momentum, wd, rescale, ctx->stream, scale));
}
extern "C" int tn_dbg_adam(tn_ctx *ctx, float *w, const float *g, float *m, float *v, int64_t n, float lr, float beta1, float beta2,
                           float epsilon, int64_t step, const float *scale) {
  TN_REQUIRE(ctx && w && g && m && v, "tn_dbg_adam: null argument");
  TN_REQUIRE(n > 0 && step > 0, "tn_dbg_adam: n and step must be positive");
  TN_ON_DEVICE(ctx->device);
  return dbg_finish(ctx, launch_adam(w, g, m, v, (long)n, lr, beta1, beta2, epsilon, (long)step, ctx->stream, scale));
}
extern "C" int tn_dbg_stage_frames(tn_ctx *ctx, const float *x, const int32_t *valid_len, int B, int T, int64_t frame_floats, float *y) {
  TN_REQUIRE(ctx && x && valid_len && y, "tn_dbg_stage_frames: null argument");
  TN_REQUIRE(B > 0 && T > 0 && frame_floats > 0, "tn_dbg_stage_frames: B, T and frame_floats must be positive");
  TN_REQUIRE(frame_floats % 4 == 0, "tn_dbg_stage_frames: frame_floats must be a multiple of 4");
  TN_ON_DEVICE(ctx->device);
  return dbg_finish(ctx, launch_stage_frames(x, valid_len, B, T, (long)frame_floats, y, ctx->stream));
}
extern "C" int tn_dbg_transpose(tn_ctx *ctx, const float *src, int rows, int cols, float *dst) {
  TN_REQUIRE(ctx && src && dst, "tn_dbg_transpose: null argument");
  TN_REQUIRE(rows > 0 && cols > 0, "tn_dbg_transpose: rows and cols must be positive");
  TN_ON_DEVICE(ctx->device);
  return dbg_finish(ctx, launch_transpose_f32(src, rows, cols, dst, ctx->stream));
}

// ---- the fp32x3 encoder mode's kernel (dense_fp32x3.hip) and, on the same operands, the fp32 mode's (dense_fp32.hip) ----
extern "C" int tn_dbg_conv_fp32x3(tn_ctx *ctx, int which, int kind, int tile, int layout, const void *x, int ldx, int K, const float *s,
                                  const float *t, const float *w_host, int N, const float *es, const float *et, float *y, int ldy, int yoff,
                                  int64_t M, int H, int W, int Ho, int Wo) {
  TN_REQUIRE(ctx && x && w_host && y, "tn_dbg_conv_fp32x3: null argument");
  TN_REQUIRE(which == 0 || which == 1, "tn_dbg_conv_fp32x3: which must be 0 (fp32x3) or 1 (fp32)");
  TN_REQUIRE(kind >= FP32_STEM && kind <= FP32_TRANS, "tn_dbg_conv_fp32x3: unknown kind");
  TN_REQUIRE(layout >= 0 && layout <= 2, "tn_dbg_conv_fp32x3: unknown input layout");
  TN_REQUIRE(M > 0 && K > 0 && N > 0 && N % 32 == 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && M % ((int64_t)Ho * Wo) == 0,
             "tn_dbg_conv_fp32x3: bad shape (M = B Ho Wo, N a multiple of 32)");
  if (kind == FP32_STEM) {
    TN_REQUIRE(K == 147 && es && et && Ho == (H - 1) / 2 + 1 && Wo == (W - 1) / 2 + 1, "tn_dbg_conv_fp32x3: the stem has K = 147, an epilogue and a ((H - 1) / 2 + 1) x ((W - 1) / 2 + 1) output");
  } else {
    // (K a multiple of 32 and the tile selector's range are the launchers' own refusals: "conv_fp32: ..." / "conv_fp32x3: ...")
    TN_REQUIRE(s && t && !es && !et && ldx % 4 == 0, "tn_dbg_conv_fp32x3: s / t, no epilogue, ldx a multiple of 4");
    TN_REQUIRE(kind == FP32_3X3 ? (K == 1152 && ldx == 128) : ldx >= K, "tn_dbg_conv_fp32x3: K beyond the channel stride (3x3: K = 1152, ldx = 128)");
    TN_REQUIRE(kind == FP32_TRANS ? (2 * Ho <= H && 2 * Wo <= W) : (Ho == H && Wo == W), "tn_dbg_conv_fp32x3: output map size does not fit the input's");
  }
  TN_ON_DEVICE(ctx->device);
  const int kp = (K + 31) / 32 * 32;
  std::vector<float> wk((size_t)kp * N, 0.f);
  memcpy(wk.data(), w_host, (size_t)K * N * sizeof(float));
  float *wd = nullptr;
  uint16_t *wx = nullptr;
  if (which == 0) wx = up(fp32x3_pack_weights(wk.data(), kp, N));
  else wd = up(wk);
  TN_REQUIRE(wd || wx, "tn_dbg_conv_fp32x3: device allocation failed");
  Fp32ConvArgs a{};
  a.kind = kind; a.x = x; a.layout = layout; a.ldx = ldx; a.K = K; a.s = s; a.t = t; a.w = wd; a.wx = wx; a.N = N; a.es = es; a.et = et;
  a.y = y; a.ldy = ldy; a.yoff = yoff; a.M = (long)M; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo;
  const int rc = which == 0 ? launch_conv_fp32x3(a, ctx->stream, tile) : launch_conv_fp32(a, ctx->stream, tile);
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(wd); (void)hipFree(wx);
  if (rc) return rc;
  TN_HIP_CHECK(e);
  return TN_OK;
}

// The fp32 mode's max pool (dense_fp32.hip) on caller buffers
extern "C" int tn_dbg_maxpool_fp32(tn_ctx *ctx, const float *x, int B, int H, int W, float *y, int ldy, int Ho, int Wo) {
  TN_REQUIRE(ctx && x && y, "tn_dbg_maxpool_fp32: null argument");
  TN_REQUIRE(B > 0 && H > 0 && W > 0, "tn_dbg_maxpool_fp32: B, H and W must be positive");
  TN_REQUIRE(Ho == (H - 1) / 2 + 1 && Wo == (W - 1) / 2 + 1, "tn_dbg_maxpool_fp32: the output is ((H - 1) / 2 + 1) x ((W - 1) / 2 + 1)");
  TN_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "tn_dbg_maxpool_fp32: buffers must be 16-byte aligned");
  TN_ON_DEVICE(ctx->device);
  return dbg_finish(ctx, launch_maxpool_fp32(x, B, H, W, y, ldy, Ho, Wo, ctx->stream));
}

// The latency GEMM's launchers on caller operands.  form 0: launch_linear_f32_lat2 (row-major X and W); 1: launch_linear_f32_lat_wk4
// on the k-group-major copy of W built here, X row-major (ldx > 0) or k-group-major with -ldx >= M rows.
extern "C" int tn_dbg_linear_lat(tn_ctx *ctx, int form, const float *X, int ldx, const float *W, int ldw, const float *bias, float *Y, int ldy,
                                 int M, int N, int K, int nsplit, int K2, int *route) {
  TN_REQUIRE(ctx && X && W && Y, "tn_dbg_linear_lat: null argument");
  TN_REQUIRE(form == 0 || form == 1, "tn_dbg_linear_lat: form must be 0 (lat / lat2) or 1 (lat_wk4)");
  TN_REQUIRE(M >= 1 && N >= 1 && K >= 1 && M <= 65535 * 16 && N <= (1 << 20) && K <= (1 << 20), "tn_dbg_linear_lat: needs M, N, K >= 1");
  TN_REQUIRE(ldw >= K && ldy >= N, "tn_dbg_linear_lat: ldw below K or ldy below N");
  TN_REQUIRE(form == 0 ? ldx >= K : (ldx >= K || -ldx >= M), "tn_dbg_linear_lat: ldx below K (row-major) or X's rows below M (k-group-major)");
  TN_ON_DEVICE(ctx->device);
  hipStream_t s = ctx->stream;
  if (form == 0) {
    TN_REQUIRE(nsplit >= N || (nsplit >= 16 && nsplit % 16 == 0 && K2 > 0 && K2 <= K && K2 % 4 == 0), "tn_dbg_linear_lat: bad column split");
    if (route) *route = linear_f32_lat_takes(X, ldx, W, ldw, M, N, K) ? 0 : 2;
    if (int rc = launch_linear_f32_lat2(X, ldx, W, ldw, bias, Y, ldy, M, N, K, nsplit, K2, s)) return rc;
    TN_HIP_CHECK(hipStreamSynchronize(s));
    return TN_OK;
  }
  TN_REQUIRE(nsplit >= N, "tn_dbg_linear_lat: the k-group-major form has no column split");
  TN_REQUIRE((ldx < 0 || (ldx & 3) == 0) && (K & 3) == 0 && ((uintptr_t)X & 15) == 0, "tn_dbg_linear_lat: the k-group-major form needs float4-aligned operands");
  std::vector<float> w((size_t)N * K);
  TN_HIP_CHECK(hipMemcpy2DAsync(w.data(), sizeof(float) * K, W, sizeof(float) * ldw, sizeof(float) * K, N, hipMemcpyDeviceToHost, s));
  TN_HIP_CHECK(hipStreamSynchronize(s));
  const std::vector<float> wk = pack_wk4(w.data(), N, K);
  float *wk4 = nullptr;
  TN_HIP_CHECK(hipMalloc((void **)&wk4, sizeof(float) * wk.size()));
  hipError_t e = hipMemcpyAsync(wk4, wk.data(), sizeof(float) * wk.size(), hipMemcpyHostToDevice, s);
  int rc = TN_OK;
  if (e == hipSuccess) rc = launch_linear_f32_lat_wk4(X, ldx, wk4, bias, Y, ldy, M, N, K, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  (void)hipFree(wk4);
  TN_HIP_CHECK(e);
  TN_HIP_CHECK(e2);
  if (route) *route = 1;
  return rc;
}
