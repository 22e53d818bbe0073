// Test hooks of the captioner's kernels (include/tennis_hip_debug.h): each runs one kernel of gnmt_kernels.hip on caller operands
// through the launcher the decoder / the training step calls, so a hook's launch is the production launch.
#include <vector>

#include "gnmt_kernels.h"
#include "train.h"

#ifdef TN_DEC_STAMPS
extern "C" int tn_dbg_dec_stamps(long long *out) { return read_dec_stamps(out); }
#endif

extern "C" int tn_dbg_gnmt_attention_fwd(tn_ctx *ctx, const float *g0, const float *hprev, int ldh, const float *cprev, int lstm,
                                         const float *keyproj, const float *mem, const int32_t *valid_len, int B, int T, int H, int beam,
                                         int split_cap, float *hn, float *cn, float *x1, int ldx1, float *ctx_out, float *w_out) {
  TN_REQUIRE(ctx && g0 && hprev && keyproj && mem && valid_len && hn && x1 && ctx_out && w_out, "tn_dbg_gnmt_attention_fwd: null argument");
  TN_REQUIRE(!lstm || (cprev && cn), "tn_dbg_gnmt_attention_fwd: the LSTM form needs cprev and cn");
  TN_REQUIRE(B >= 1 && T >= 1 && beam >= 1 && H >= 4 && H % 4 == 0 && (long)B * beam <= 65535,
             "tn_dbg_gnmt_attention_fwd: needs B, T, beam >= 1 and H a positive multiple of 4");
  TN_REQUIRE(ldh >= H && ldx1 >= 2 * H, "tn_dbg_gnmt_attention_fwd: ldh below H or ldx1 below 2 H");
  TN_REQUIRE(split_cap == 0 || split_cap == 16 || split_cap == 8 || split_cap == 4 || split_cap == 2 || split_cap == 1,
             "tn_dbg_gnmt_attention_fwd: split_cap must be 0, 16, 8, 4, 2 or 1");
  TN_REQUIRE(att_split(T, H, kStepLdsMax) > 0, "tn_dbg_gnmt_attention_fwd: 3 * max(hidden, source length) floats exceed the step kernel's 152 KiB of LDS");
  TN_ON_DEVICE(ctx->device);
  hipStream_t s = ctx->stream;
  float *kpT = nullptr;
  TN_HIP_CHECK(hipMalloc((void **)&kpT, sizeof(float) * (size_t)B * H * ((T + 3) & ~3)));
  DecAttentionArgs a;
  a.g0 = g0; a.hprev = hprev; a.ldh = ldh; a.cprev = cprev; a.lstm = lstm != 0; a.hn = hn; a.cn = lstm ? cn : nullptr; a.x1 = x1; a.ldx1 = ldx1;
  a.kpT = kpT; a.mem = mem; a.valid_len = valid_len; a.ctx = ctx_out; a.beam = beam; a.R = B * beam; a.T = T; a.H = H; a.wsave = w_out; a.wpitch = T;
  a.split_cap = split_cap;
  int rc = launch_transpose_bth(keyproj, kpT, B, T, H, s);
  if (!rc) rc = launch_dec_attention(a, s);
  const hipError_t e = hipStreamSynchronize(s);
  (void)hipFree(kpT);
  if (rc) return rc;
  TN_HIP_CHECK(e);
  return TN_OK;
}

extern "C" int tn_dbg_gnmt_attention_bwd(tn_ctx *ctx, const float *aw, const float *mem, const float *keyproj, const float *c0, int lc0,
                                         const float *c1, int lc1, const int32_t *valid_len, int B, int T, int H, float *ds, float *dctx,
                                         float *dh0) {
  TN_REQUIRE(ctx && aw && mem && keyproj && (c0 || c1) && valid_len && ds && dctx && dh0, "tn_dbg_gnmt_attention_bwd: null argument");
  TN_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && H >= 4 && H % 4 == 0, "tn_dbg_gnmt_attention_bwd: needs B, T >= 1 and H a positive multiple of 4");
  TN_REQUIRE((!c0 || lc0 >= H) && (!c1 || lc1 >= H), "tn_dbg_gnmt_attention_bwd: an addend's pitch is below H");
  TN_ON_DEVICE(ctx->device);
  TN_TRY(launch_trn_att_bwd(aw, mem, keyproj, c0, lc0, c1, lc1, valid_len, ds, dctx, dh0, B, T, H, ctx->stream));      // (refuses T, H beyond the LDS)
  TN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return TN_OK;
}

extern "C" int tn_dbg_gnmt_attention_outer(tn_ctx *ctx, const float *aw, const float *ds, const float *dctx, const float *h0, int ldh, int steps,
                                           int B, int T, int H, float *dmem, float *dkp) {
  TN_REQUIRE(ctx && aw && ds && dctx && h0 && dmem && dkp, "tn_dbg_gnmt_attention_outer: null argument");
  TN_REQUIRE(steps >= 1 && B >= 1 && B <= 65535 && T >= 1 && H >= 4 && H % 4 == 0,
             "tn_dbg_gnmt_attention_outer: needs steps, B, T >= 1 and H a positive multiple of 4");
  TN_REQUIRE(ldh >= H, "tn_dbg_gnmt_attention_outer: ldh below H");
  TN_ON_DEVICE(ctx->device);
  TN_TRY(launch_trn_att_outer(aw, ds, dctx, h0, ldh, dmem, dkp, steps, B, T, H, ctx->stream));
  TN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return TN_OK;
}

extern "C" int tn_dbg_gnmt_ce(tn_ctx *ctx, const float *logits, const int32_t *labels, int ld, const int32_t *valid_len, int B, int L, int V,
                              float *dlogits, float *loss_rows, float *loss, float *masked_loss) {
  TN_REQUIRE(ctx && logits && labels && valid_len && dlogits && loss_rows && loss && masked_loss, "tn_dbg_gnmt_ce: null argument");
  TN_REQUIRE(B >= 1 && B <= 65535 && L >= 1 && V >= 1, "tn_dbg_gnmt_ce: needs B, L, V >= 1");
  TN_REQUIRE(ld >= L, "tn_dbg_gnmt_ce: the labels' pitch is below L");
  TN_ON_DEVICE(ctx->device);
  hipStream_t s = ctx->stream;
  TN_TRY(launch_trn_ce_bwd(logits, labels, ld, valid_len, B, L, V, dlogits, loss_rows, s));
  TN_TRY(launch_colsum_f32(loss_rows, 1, L * B, 1, loss, s));
  TN_TRY(launch_masked_ce(logits, labels, ld, valid_len, masked_loss, B, L, V, s));
  TN_HIP_CHECK(hipStreamSynchronize(s));
  return TN_OK;
}

extern "C" int tn_dbg_gnmt_emb_grad(tn_ctx *ctx, const float *dx0, int K0, const int32_t *tgt, int ld, int B, int L, int E, int V, float *demb) {
  TN_REQUIRE(ctx && dx0 && tgt && demb, "tn_dbg_gnmt_emb_grad: null argument");
  TN_REQUIRE(B >= 1 && L >= 1 && E >= 1 && V >= 1, "tn_dbg_gnmt_emb_grad: needs B, L, E, V >= 1");
  TN_REQUIRE(K0 > E && ld >= L, "tn_dbg_gnmt_emb_grad: K0 must exceed E and the tokens' pitch must reach L");
  TN_ON_DEVICE(ctx->device);
  TN_TRY(launch_trn_emb_grad(dx0, K0, tgt, ld, B, L, E, V, demb, ctx->stream));
  TN_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return TN_OK;
}

// One launch of dec_beam_kernel<NBM> on caller operands through launch_dec_beam: the instantiation, LDS, projection split and extra
// workgroups are the ones gnmt_beam_search gets for the shape.  wp / bp HOST (packed by pack_proj as tn_gnmt_create packs them), everything else DEVICE.
extern "C" int tn_dbg_gnmt_beam_step(tn_ctx *ctx, const float *g1, float *x1, int ldx1, int lstm, float *c1cur, const float *wp_host,
                                     const float *bp_host, int B, int H, int E, int V, int beam, int step, float lp, float prev_lp, int eos,
                                     int split_cap, float *scores, int32_t *alive, int32_t *vlen, int32_t *bp_par, int32_t *bp_word,
                                     int32_t *any_alive, float *hstate, int32_t *parent_out, int32_t *tok_out, const float *w1x,
                                     const float *b1x, int K1p, float *p0, const float *emb, const float *ctxv, const float *h0n,
                                     const float *c0n, float *x0, float *c0cur) {
  TN_REQUIRE(ctx && g1 && x1 && wp_host && scores && alive && vlen && bp_par && bp_word && any_alive, "tn_dbg_gnmt_beam_step: null argument");
  TN_REQUIRE(!lstm || c1cur, "tn_dbg_gnmt_beam_step: the LSTM form needs c1cur");
  TN_REQUIRE(beam >= 1 && beam <= 16, "tn_dbg_gnmt_beam_step: beam must be 1 to 16");
  TN_REQUIRE(B >= 1 && B <= 4096 && H >= 4 && H % 4 == 0 && H <= 4096 && E >= 1 && V >= beam && V <= 65536 && step >= 1 && lp > 0.f,
             "tn_dbg_gnmt_beam_step: needs 1 <= B <= 4096, H a positive multiple of 4, E >= 1, beam <= V <= 65536, step >= 1, lp > 0");
  const int R = B * beam;
  TN_REQUIRE(ldx1 >= 3 * H || -ldx1 >= R, "tn_dbg_gnmt_beam_step: x1's pitch is below 3 H (row-major) or its rows below B * beam (k-group-major)");
  TN_REQUIRE(split_cap == 0 || split_cap == 16 || split_cap == 8 || split_cap == 4 || split_cap == 2 || split_cap == 1,
             "tn_dbg_gnmt_beam_step: split_cap must be 0, 16, 8, 4, 2 or 1");
  if (tok_out) {       // the token form; p0 == NULL: without the extra workgroups
    TN_REQUIRE(!emb && !ctxv && !h0n && !c0n && !x0 && !c0cur, "tn_dbg_gnmt_beam_step: the token form takes no x0 operands");
    TN_REQUIRE(p0 ? (w1x && b1x) : (!w1x && !b1x), "tn_dbg_gnmt_beam_step: p0, w1x and b1x come together");
    TN_REQUIRE(!p0 || (K1p >= 2 * H && K1p % 4 == 0 && (ldx1 < 0 || ldx1 % 4 == 0) && (((uintptr_t)x1 | (uintptr_t)w1x) & 15) == 0),
               "tn_dbg_gnmt_beam_step: the p0 tiles need K1p >= 2 H and float4-aligned x1, w1x and pitches");
  } else {
    TN_REQUIRE(!w1x && !b1x && !p0, "tn_dbg_gnmt_beam_step: the x0 form takes no p0 operands");
    TN_REQUIRE(emb && ctxv && h0n && x0 && (!lstm || (c0n && c0cur)), "tn_dbg_gnmt_beam_step: the x0 form needs emb, ctx, h0n, x0 (LSTM: c0n, c0cur)");
  }
  int bsplit = beam_split(H, V, beam, kStepLdsMax);
  if (split_cap && split_cap < bsplit) bsplit = split_cap;
  TN_REQUIRE(beam_lds_bytes(H, V, beam, bsplit) <= kStepLdsMax,
             "tn_dbg_gnmt_beam_step: beam * (2*hidden + 2*vocab) floats exceed the step kernel's 152 KiB of LDS");
  TN_ON_DEVICE(ctx->device);
  hipStream_t s = ctx->stream;
  std::vector<float> wt, bpad;
  pack_proj(wp_host, bp_host, V, H, wt, bpad);
  float *wpT = nullptr, *bpp = nullptr;
  hipError_t e = hipMalloc((void **)&wpT, sizeof(float) * wt.size());
  if (e == hipSuccess) e = hipMalloc((void **)&bpp, sizeof(float) * bpad.size());
  if (e == hipSuccess) e = hipMemcpyAsync(wpT, wt.data(), sizeof(float) * wt.size(), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(bpp, bpad.data(), sizeof(float) * bpad.size(), hipMemcpyHostToDevice, s);
  int rc = TN_OK;
  if (e == hipSuccess) {
    DecBeamArgs a;
    a.g1 = g1; a.x1 = x1; a.K1 = ldx1; a.lstm = lstm != 0; a.c1cur = c1cur; a.wpT = wpT; a.bp = bpp; a.h0n = h0n; a.ctx = ctxv; a.c0n = c0n;
    a.x0 = x0; a.c0cur = c0cur; a.emb = emb; a.B = B; a.H = H; a.E = E; a.V = V; a.beam = beam; a.step = step; a.lp = lp; a.prev_lp = prev_lp;
    a.eos = eos; a.scores = scores; a.alive = alive; a.vlen = vlen; a.bp_par = bp_par; a.bp_word = bp_word; a.any_alive = any_alive;
    a.hstate = hstate; a.parent_out = parent_out; a.tok_out = tok_out; a.w1x = w1x; a.b1x = b1x; a.K1p = K1p; a.p0 = p0; a.split_cap = split_cap;
    rc = launch_dec_beam(a, s);
  }
  const hipError_t e2 = hipStreamSynchronize(s);
  (void)hipFree(wpT);
  (void)hipFree(bpp);
  if (rc) return rc;
  TN_HIP_CHECK(e);
  TN_HIP_CHECK(e2);
  return TN_OK;
}
