// Launchers and host-side planners of the captioner's kernels (gnmt_kernels.hip): what the inference handle (captioner.hip), the
// training handle (captioner_train.hip) and the test hooks (gnmt_dbg.hip) launch.  Every launcher enqueues on `s` and returns a TN_ code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "common.h"

// ---- the step kernels' launch parameters: 1024 threads = 16 waves ----
constexpr int kBeamThreads = 1024;
// dynamic LDS the step kernels may ask for: a launch above 64 KiB needs the kernel's limit raised first (160 KiB per CU on
// gfx950; 8 KiB are left for the kernels' static arrays)
constexpr size_t kStepLdsMax = 152 * 1024;
// Work split of the step kernels' three streaming loops (attention scores, attention context, vocabulary projection): a
// thread owns FOUR consecutive outputs (one 16-byte load per operand row) and a slice of the contraction; n4 groups of four
// outputs are dealt over 64 / 128 / 256 threads and the remaining factor of the 1024 threads (16 / 8 / 4) splits the
// contraction, the partial sums meet in LDS.  Each of these loops used to be one scalar load + one LDS read per FMA row:
// the LDS pipe (every lane reading the same broadcast value) and the number of loads in flight bound them, not the bytes.
// `split` (16, 8, 4, 2 or 1) caps the number of partial sums: the host lowers it when 16 partial rows do not fit the LDS
// (a wide beam with a large vocabulary, a very long source).
__device__ __host__ __forceinline__ int step_groups(int n4, int split) {
  const int g = n4 <= 64 ? 64 : n4 <= 128 ? 128 : 256, floor_g = 1024 / split;
  return g > floor_g ? g : floor_g;
}
inline size_t att_lds_bytes(int T, int H, int split) {      // q[H] | w[Tp] | part[partials * max(Tp, H)]
  const int Tp = (T + 3) & ~3;
  const int hg = 1024 / step_groups(Tp / 4, split), sg = 1024 / step_groups(H / 4, split);
  const size_t a = (size_t)hg * Tp, b = (size_t)sg * H;
  return ((size_t)H + Tp + (a > b ? a : b)) * sizeof(float);
}
// dynamic LDS of trn_att_bwd_kernel: dctx[H] | ds[T] | part[16][H] | red[16]
inline size_t att_bwd_lds_bytes(int T, int H) { return (size_t)(17 * H + T + 16) * sizeof(float); }
// the largest split whose attention kernel fits the step kernels' LDS (0: not even one partial row does)
inline int att_split(int T, int H, size_t limit) {
  for (int sp = 16; sp >= 1; sp >>= 1)
    if (att_lds_bytes(T, H, sp) <= limit) return sp;
  return 0;
}
// dec_beam_kernel's launch parameters: the instantiation (beam rows a projection thread carries), the dynamic LDS
// h1n[H][NP] | c1n[H][NP] | logits[beam * Vp] | part[KQ * beam * Vp] (+ 16) for a projection split, and the largest split that
// fits `limit` (1 where none does: the caller compares beam_lds_bytes with its limit)
inline int beam_nbm(int beam) { return beam <= 4 ? 4 : beam == 5 ? 5 : beam <= 8 ? 8 : 16; }   // beam 5: the reference's flag default
inline size_t beam_lds_bytes(int H, int V, int beam, int split) {
  const int nbm = beam_nbm(beam), Vp = (V + 3) & ~3;
  return ((size_t)2 * ((nbm + 3) & ~3) * H + (size_t)(1 + kBeamThreads / step_groups(Vp / 4, split)) * beam * Vp + 16) * sizeof(float);
}
inline int beam_split(int H, int V, int beam, size_t limit) {
  int sp = 16;
  while (sp > 1 && beam_lds_bytes(H, V, beam, sp) > limit) sp >>= 1;
  return sp;
}
// the p0 tiles beside the clips (dec_beam_kernel, `tok_out`): workgroups of four 16 x 16 tiles over (R, 4H), and the LDS their
// partial sums need
inline int beam_gemm_wgs(int R, int H) { return (((R + 15) / 16) * (4 * H / 16) + 3) / 4; }
constexpr size_t kBeamTileLds = 4 * 4 * 64 * 4 * sizeof(float);
// the vocabulary projection as dec_beam_kernel reads it: wt = Wp^T (H, Vp) and bpad (Vp), Vp = V rounded up to 4 (the kernel loads
// four columns at a time), the pad columns zero; wp (V,H) row-major, bp (V) or NULL (no bias)
void pack_proj(const float *wp, const float *bp, int V, int H, std::vector<float> &wt, std::vector<float> &bpad);
// a weight matrix w (N rows of K, K % 4 == 0) k-group-major, [k / 4][N][4]: the operand form of lat_tile_f32<true> (linear.h)
std::vector<float> pack_wk4(const float *w, int N, int K);

// ---- the two step kernels: operands by name, absent ones null (the kernels' comments in gnmt_kernels.hip say what each is).
// The launchers pick the split (the largest that fits kStepLdsMax, lowered to split_cap when that is non-zero: the test hooks),
// the LDS and, for dec_beam_kernel, the instantiation and the extra p0 workgroups; a shape beyond the LDS is TN_ERR_INVALID. ----
struct DecAttentionArgs {
  const float *g0 = nullptr, *hprev = nullptr, *cprev = nullptr, *kpT = nullptr, *mem = nullptr, *ew = nullptr, *p0 = nullptr;
  const int32_t *valid_len = nullptr, *tok = nullptr, *par = nullptr;
  float *hn = nullptr, *cn = nullptr, *x1 = nullptr, *ctx = nullptr, *wsave = nullptr;
  int ldh = 0, ldx1 = 0, beam = 1, R = 0, T = 0, H = 0, split_cap = 0;       // R = clips * beam decoder rows, one workgroup each
  long wpitch = 0;
  bool lstm = false;
};
int launch_dec_attention(const DecAttentionArgs &a, hipStream_t s);
struct DecBeamArgs {
  const float *g1 = nullptr, *wpT = nullptr, *bp = nullptr, *h0n = nullptr, *ctx = nullptr, *c0n = nullptr, *emb = nullptr;      // g1 (B * beam, 4H)
  float *x1 = nullptr, *c1cur = nullptr, *x0 = nullptr, *c0cur = nullptr, *scores = nullptr, *hstate = nullptr;
  int32_t *alive = nullptr, *vlen = nullptr, *bp_par = nullptr, *bp_word = nullptr, *any_alive = nullptr, *parent_out = nullptr, *tok_out = nullptr;
  int K1 = 0, B = 0, H = 0, E = 0, V = 0, beam = 0, step = 0, eos = 0, split_cap = 0;
  float lp = 1.f, prev_lp = 1.f;
  bool lstm = false;
  // p0 != NULL (with tok_out): extra workgroups compute p0 (R, 4H) = x1[:, 0:2H] . w1x^T + b1x, w1x of pitch K1p
  const float *w1x = nullptr, *b1x = nullptr;
  float *p0 = nullptr;
  int K1p = 0;
};
int launch_dec_beam(const DecBeamArgs &a, hipStream_t s);

// ---- decoder steps around them ----
int launch_transpose_bth(const float *src, float *dst, int B, int T, int H, hipStream_t s);
// a step's inputs for rows r < R, source row r / beam: x0[r] = [embed(tok), ctx_prev | 0 (NULL), h0_prev], x1[r, 2H:3H] = h1_prev
// (x1: pitch ldx1 as xidx reads it), and with c0_prev the cell states c0cur / c1cur = c0_prev / c1_prev (pitch H);
// tok = tgt[r * ld + col], or col where tgt is NULL
int launch_dec_prep(const float *emb, const int32_t *tgt, int ld, int col, const float *ctx_prev, int ldc, const float *h0_prev, int ld0,
                    const float *h1_prev, int ld1, const float *c0_prev, const float *c1_prev, float *x0, float *x1, int ldx1, float *c0cur,
                    float *c1cur, int beam, int R, int H, int E, hipStream_t s);
// a cell behind the attention on g (R,4H), x (R,3H) = [layer input, attention, h_prev]: new state -> hn (+ cn), every output optional:
// out[r * ldo + u] = h (* mask) (+ x's layer input with residual), att_dst[r * ldo + u] = x's attention columns
int launch_dec_cell(const float *g, const float *x, bool lstm, const float *cprev, float *hn, float *cn, const float *mask, bool residual,
                    float *out, int ldo, float *att_dst, int R, int H, hipStream_t s);
int launch_dec_mid_state(const int32_t *parent, const float *hn, const float *cn, float *x, float *ccur, bool from_clip, int beam, int R, int H,
                         hipStream_t s);
// y[i] = x[i] (* m[i]) (+ r[i]), i < n (m, r optional; y may be x);  out[r * ldo + u] = a[r * la + u] (* m[r * H + u]) (+ b[r * lb + u])
int launch_mul_add(const float *x, const float *m, const float *r, float *y, long n, hipStream_t s);
int launch_mul_add_rows(const float *a, int la, const float *m, const float *b, int lb, float *out, int ldo, int R, int H, hipStream_t s);

// ---- beam search bookkeeping ----
int launch_beam_init(float *scores, int32_t *alive, int32_t *vlen, int32_t *tok, int32_t *samples, int L, int B, int beam, int bos, hipStream_t s);
int launch_beam_samples(const int32_t *bp_par, const int32_t *bp_word, int32_t *samples, int L, int steps, int B, int beam, int bos, hipStream_t s);
int launch_beam_finalize(const int32_t *alive, int32_t *vlen, int32_t *samples, int L, int last, int R, int eos, hipStream_t s);
// attention (B * beam, LA, T) of the final hypotheses from the steps' history hist (steps, R, T); rowtab: (R, steps) scratch
int launch_beam_attention(const int32_t *bp_par, const int32_t *bp_word, const float *hist, int32_t *rowtab, float *attention, int steps, int B,
                          int beam, int T, int LA, hipStream_t s);

// ---- losses and the training step ----
int launch_masked_ce(const float *logits, const int32_t *labels, int ldl, const int32_t *valid_len, float *loss, int B, int L, int V, hipStream_t s);
int launch_trn_ce_bwd(const float *logits, const int32_t *labels, int ldl, const int32_t *valid_len, int B, int L, int V, float *dlogits,
                      float *loss_rows, hipStream_t s);
// dh = the sum of the non-null addends a0 .. a3 (row strides l0 .. l3)
int launch_trn_gru_bwd(const float *g, const float *hprev, int ldh, const float *a0, int l0, const float *a1, int l1, const float *a2, int l2,
                       const float *a3, int l3, float *dg, float *dhz, int R, int H, hipStream_t s);
int launch_trn_lstm_bwd(const float *g, const float *cprev, const float *cnew, const float *a0, int l0, const float *a1, int l1, const float *a2,
                        int l2, const float *a3, int l3, const float *dcc, float *dg, float *dhz, float *dcz, int R, int H, hipStream_t s);
int launch_trn_att_bwd(const float *aw, const float *mem, const float *keyproj, const float *c0, int lc0, const float *c1, int lc1,
                       const int32_t *valid_len, float *ds, float *dctx, float *dh0, int B, int T, int H, hipStream_t s);
int launch_trn_att_outer(const float *aw, const float *ds, const float *dctx, const float *h0, int ldh, float *dmem, float *dkp, int steps, int B,
                         int T, int H, hipStream_t s);
int launch_trn_emb_grad(const float *dx0, int K0, const int32_t *tgt, int ld, int B, int L, int E, int V, float *demb, hipStream_t s);
int launch_trn_stack(const float *wi, const float *wh, const float *bi, const float *bh, int in, int H, bool lstm, float *wc, float *bc, hipStream_t s);
int launch_trn_unstack(const float *dwc, const float *dbc, int in, int H, bool lstm, float *dwi, float *dwh, float *dbi, float *dbh, hipStream_t s);
int launch_trn_dropout_mask(float *mask, long n, float p, unsigned long long key, hipStream_t s);
int launch_trn_dec_len(const int32_t *tgt_vl, int32_t *out, int B, hipStream_t s);
#ifdef TN_DEC_STAMPS
int read_dec_stamps(long long *out);      // tuning builds: the 24 phase stamps of the step kernels' workgroup 0
#endif
