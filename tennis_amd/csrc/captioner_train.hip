// GNMT captioner, training handle, fp32 throughout; the kernels and their launchers: gnmt_kernels.hip.
// Teacher-forced forward with everything the backward pass needs kept per step (step-major (L,B,.) arrays), the
// gradient of the token-averaged masked cross-entropy, back-propagation through the decoder steps, the attention, the
// key projection and the encoder layers, Adam.  Reference: train_gnmt.py:310,328-337.
// Round 4: any num_layers >= 2 with num_bi_layers < num_layers and use_residual, as the reference passes them into the model it
// trains (train_gnmt.py:58-61,223-227; gnmt.py:71-111,136-160,369-404).  Every encoder / decoder layer is a record of its
// parameter offsets, the forward state kept for the backward pass and its backward workspace; the step below walks the records.
#include <vector>

#include "api_internal.h"
#include "gnmt_kernels.h"
#include "linear.h"
#include "rnn.h"
#include "train.h"

namespace {

struct TrnEnc : CellOffsets {   // encoder layer i: bidirectional (i < num_bi_layers: in -> 2H) or uni-directional (in -> H)
  // (the offsets: the directions adjacent per tensor kind - one GEMM / one recurrent launch serves both)
  int in, D, out;        // input width, directions, output width D * H
  bool res;              // use_residual && i > num_bi_layers (gnmt.py:155-157)
  float *whT, *wiT;      // per direction (H, GH); (in, D GH) [layers behind the first]
  float *gi, *seq, *sav, *hl, *cl, *M, *xn;       // xn: what the next layer (or the attention) reads = dropout(seq) (+ input)
  float *dxn, *dseq, *dgi, *dgh, *hp, *dhl, *dcl; // dxn: gradient w.r.t. xn
};
struct TrnDec : CellOffsets {   // decoder cell j: step input x = [embedding | layer input, attention, h_prev], K = in + H columns
  int in, K;
  float *wc, *bc, *wcT;  // stacked (4H, K) step matrix, its bias, its transpose
  float *X, *G, *C, *Hs, *M;       // per step (L, B, .): inputs, stacked pre-activations, cell states (LSTM), states h (j >= 1), dropout masks (j >= 1)
  float *dG, *dX, *dhz, *dcz, *dW, *db;
};

}  // namespace

struct tn_gnmt_trainer : TrainParams {
  int F, H, E, V, maxB, maxT, maxL, NL, NBI;
  bool residual;
  int G;                          // gates per cell: 3 GRU, 4 LSTM
  long step;
  long o_wk, o_wp, o_bp, o_emb;
  float *am, *av;                 // Adam's moments, next to the parameters w and the gradients g
  std::vector<TrnEnc> enc;
  std::vector<TrnDec> dec;
  float *wpT, *wkT;
  float *DS, *DCTX;          // per decoder step: the attention scores' gradient (L,B,T) and the context's (L,B,H)
  float *keyproj, *keyprojT, *AW, *h0tmp, *ctxtmp, *logits, *lossrows, *Out, *dlog, *dOut, *dq, *dkp, *tmpA, *tmpB, *tmpM, *tmpAtt;
  int32_t *vl, *tvl;
  float drop_p;
  unsigned long long drop_seed, drop_count;
};

static int trainer_refresh(tn_gnmt_trainer *t) {
  hipStream_t s = t->ctx->stream;
  const int H = t->H, V = t->V, GH = t->G * H;
  for (size_t i = 0; i < t->enc.size(); ++i) {
    TrnEnc &e = t->enc[i];
    for (int d = 0; d < e.D; ++d) TN_TRY(launch_transpose_f32(t->w + e.o_wh + (long)d * GH * H, GH, H, e.whT + (long)d * H * GH, s));
    if (i > 0) TN_TRY(launch_transpose_f32(t->w + e.o_wi, e.D * GH, e.in, e.wiT, s));
  }
  for (TrnDec &d : t->dec) {
    TN_TRY(launch_trn_stack(t->w + d.o_wi, t->w + d.o_wh, t->w + d.o_bi, t->w + d.o_bh, d.in, H, t->G == 4, d.wc, d.bc, s));
    TN_TRY(launch_transpose_f32(d.wc, 4 * H, d.K, d.wcT, s));
  }
  TN_TRY(launch_transpose_f32(t->w + t->o_wp, V, H, t->wpT, s));
  return launch_transpose_f32(t->w + t->o_wk, H, H, t->wkT, s);
}

extern "C" int tn_gnmt_trainer_create_ex(tn_ctx *ctx, const tn_param *params, int n_params, const char *prefix_c, tn_rnn_kind cell_kind,
                                         int input_size, int hidden, int embed, int vocab, int num_layers, int num_bi_layers, int flags,
                                         int max_batch, int max_src_len, int max_tgt_len, tn_gnmt_trainer **out) {
  TN_REQUIRE(ctx && params && prefix_c && out, "tn_gnmt_trainer_create: null argument");
  TN_REQUIRE(cell_kind == TN_RNN_GRU || cell_kind == TN_RNN_LSTM, "tn_gnmt_trainer_create: cell_type must be 'gru' or 'lstm'");
  TN_REQUIRE((flags & ~TN_GNMT_USE_RESIDUAL) == 0, "tn_gnmt_trainer_create_ex: unknown flag");
  // the same shapes tn_gnmt_create_ex serves (gnmt.py:78-80; a memory of 2H columns does not fit the attention's key width)
  TN_REQUIRE(num_layers >= 2 && num_layers <= 8 && num_bi_layers >= 0 && num_bi_layers < num_layers,
             "tn_gnmt_trainer_create: need 2 <= num_layers <= 8 and 0 <= num_bi_layers < num_layers");
  const int G_ = cell_kind == TN_RNN_GRU ? 3 : 4;
  TN_REQUIRE(input_size > 0 && hidden > 0 && hidden % 4 == 0 && G_ * hidden <= 2048 && embed > 0 && vocab > 1 && max_batch > 0 &&
                 max_src_len > 0 && max_tgt_len > 1, "tn_gnmt_trainer_create: bad shape (gates*hidden <= 2048, hidden % 4 == 0)");
  TN_ON_DEVICE(ctx->device);
  tn_gnmt_trainer *t = new tn_gnmt_trainer();
  t->ctx = ctx; t->F = input_size; t->H = hidden; t->E = embed; t->V = vocab; t->maxB = max_batch; t->maxT = max_src_len;
  t->maxL = max_tgt_len - 1; t->step = 0; t->G = G_; t->NL = num_layers; t->NBI = num_bi_layers;
  t->residual = (flags & TN_GNMT_USE_RESIDUAL) != 0;
  const long H = hidden, V = vocab, GH = (long)G_ * H;
  GnmtOffsets o;
  t->table = gnmt_param_table(G_, input_size, hidden, embed, vocab, num_layers, num_bi_layers, prefix_c, &o);
  t->n = t->table.n;
  t->o_wk = o.o_wk; t->o_wp = o.o_wp; t->o_bp = o.o_bp; t->o_emb = o.o_emb;
  t->enc.resize(num_layers); t->dec.resize(num_layers);
  for (int i = 0; i < num_layers; ++i) {
    TrnEnc &e = t->enc[i];
    static_cast<CellOffsets &>(e) = o.enc[i];
    e.in = gnmt_enc_in(i, input_size, hidden, num_bi_layers); e.D = gnmt_enc_dirs(i, num_bi_layers); e.out = e.D * hidden;
    e.res = t->residual && i > num_bi_layers;
    TrnDec &d = t->dec[i];
    static_cast<CellOffsets &>(d) = o.dec[i];
    d.in = gnmt_dec_in(i, hidden, embed); d.K = d.in + hidden;
  }
  auto fail = [&](int code) { t->pool.release(); delete t; return code; };
  std::vector<float> w, st;
  if (!t->table.load(ParamMap(params, n_params), w, st)) return fail(TN_ERR_MISSING);
  t->w = t->pool.upload(w);
  auto fl = [&](size_t n) { return t->pool.alloc<float>(n); };
  t->g = fl(t->n); t->am = fl(t->n); t->av = fl(t->n);
  const size_t B = max_batch, T = max_src_len, L = t->maxL, BT = B * T, LB = L * B;
  for (int i = 0; i < num_layers; ++i) {
    TrnEnc &e = t->enc[i];
    const size_t D = e.D, DG = D * GH, O = e.out;
    e.whT = fl(D * H * GH); e.wiT = i ? fl((size_t)e.in * DG) : nullptr;
    e.gi = fl(BT * DG); e.seq = fl(BT * O); e.sav = fl(D * BT * (G_ + 1) * H); e.hl = fl(D * B * H); e.cl = fl(D * B * H);
    e.M = fl(BT * O); e.xn = fl(BT * O);
    e.dxn = fl(BT * O); e.dseq = fl(BT * O); e.dgi = fl(BT * DG); e.dgh = fl(BT * DG); e.hp = fl(D * BT * H);
    e.dhl = fl(D * B * H); e.dcl = fl(D * B * H);
  }
  for (int j = 0; j < num_layers; ++j) {
    TrnDec &d = t->dec[j];
    const size_t K = d.K;
    d.wc = fl(4 * H * K); d.bc = fl(4 * H); d.wcT = fl(4 * H * K);
    d.X = fl(LB * K); d.G = fl(LB * 4 * H); d.C = fl(LB * H); d.Hs = fl(LB * H); d.M = fl(LB * H);
    d.dG = fl(LB * 4 * H); d.dX = fl(LB * K); d.dhz = fl(B * H); d.dcz = fl(B * H); d.dW = fl(4 * H * K); d.db = fl(4 * H);
  }
  t->wpT = fl(V * H); t->wkT = fl(H * H);
  t->keyproj = fl(BT * H); t->keyprojT = fl(B * ((T + 3) & ~(size_t)3) * H); t->AW = fl(LB * T); t->DS = fl(LB * T); t->DCTX = fl(LB * H); t->h0tmp = fl(B * H); t->ctxtmp = fl(B * H);
  t->logits = fl(LB * V); t->lossrows = fl(LB); t->Out = fl(LB * H); t->dlog = fl(LB * V); t->dOut = fl(LB * H); t->dq = fl(B * H);
  t->dkp = fl(BT * H); t->tmpA = fl(B * H); t->tmpB = fl(B * H); t->tmpM = fl(B * H); t->tmpAtt = fl(B * H);
  t->vl = t->pool.alloc<int32_t>(B); t->tvl = t->pool.alloc<int32_t>(B);
  t->drop_p = 0.f; t->drop_seed = 0; t->drop_count = 0;
  if (t->pool.failed) { tn_set_error("device allocation failed"); return fail(TN_ERR_NOMEM); }
  TN_HIP_CHECK(hipMemsetAsync(t->g, 0, sizeof(float) * t->n, ctx->stream));
  TN_HIP_CHECK(hipMemsetAsync(t->am, 0, sizeof(float) * t->n, ctx->stream));
  TN_HIP_CHECK(hipMemsetAsync(t->av, 0, sizeof(float) * t->n, ctx->stream));
  const int rc = trainer_refresh(t);
  if (rc) return fail(rc);
  *out = t;
  return TN_OK;
}

// the reference's flag defaults (train_gnmt.py:58-61): two layers, the first bidirectional, no residual connections
extern "C" int tn_gnmt_trainer_create(tn_ctx *ctx, const tn_param *params, int n_params, const char *prefix_c, tn_rnn_kind cell_kind,
                                      int input_size, int hidden, int embed, int vocab, int max_batch, int max_src_len,
                                      int max_tgt_len, tn_gnmt_trainer **out) {
  return tn_gnmt_trainer_create_ex(ctx, params, n_params, prefix_c, cell_kind, input_size, hidden, embed, vocab, 2, 1, 0, max_batch,
                                   max_src_len, max_tgt_len, out);
}

// One training step's forward + backward.  src (B,T,F) fp32, src_valid_len (B), tgt (B, ld) token ids with tgt_len >= 2
// columns used (inputs tgt[:, :-1], labels tgt[:, 1:]), tgt_valid_len (B) as the data loader gives it (BOS and EOS
// counted); all DEVICE buffers.  loss (1 float, device) = summed NLL of the valid target tokens / their number
// (= the scalar of train_gnmt.py:332-333); logits_out (B, tgt_len-1, V) optional.  Gradients of that loss land in the
// flat gradient buffer (tn_gnmt_trainer_buffers).
extern "C" int tn_gnmt_trainer_forward_backward(tn_gnmt_trainer *t, const float *src, const int32_t *src_valid_len,
                                                const int32_t *tgt, int ld, const int32_t *tgt_valid_len, int batch, int steps,
                                                int tgt_len, float *loss, float *logits_out) {
  return gnmt_trainer_step(t, src, src_valid_len, tgt, ld, tgt_valid_len, batch, steps, tgt_len, loss, logits_out, nullptr, 0);
}

// The source of a step that is never materialised: row b * steps + t of src is row idx[b * steps + t] of a device-resident feature
// table (n_rows, F; row stride ld), a row of zeros where the index is negative (the padding behind a clip shorter than the batch's
// longest).  Layer 0's two readers of src gather it while they stage it.
struct SrcRows {
  const float *table;
  int n_rows, ld;
  const int32_t *idx;
};
static int trainer_step(tn_gnmt_trainer *t, const float *src, const SrcRows *rows, const int32_t *src_valid_len, const int32_t *tgt, int ld,
                        const int32_t *tgt_valid_len, int batch, int steps, int tgt_len, float *loss, float *logits_out, float *dsrc, int ldd);

// ... and, with dsrc, d loss / d src (train.h): the end-to-end frame-mode step hands it to the backbone's backward.
int gnmt_trainer_step(tn_gnmt_trainer *t, const float *src, const int32_t *src_valid_len, const int32_t *tgt, int ld,
                      const int32_t *tgt_valid_len, int batch, int steps, int tgt_len, float *loss, float *logits_out, float *dsrc, int ldd) {
  TN_REQUIRE(t && src && src_valid_len && tgt && tgt_valid_len && loss, "tn_gnmt_trainer_forward_backward: null argument");
  return trainer_step(t, src, nullptr, src_valid_len, tgt, ld, tgt_valid_len, batch, steps, tgt_len, loss, logits_out, dsrc, ldd);
}

// The same step from a device-resident feature table (tennis_hip.h): everything but layer 0's two readers of src is the code above.
extern "C" int tn_gnmt_trainer_forward_backward_rows(tn_gnmt_trainer *t, const float *table, int n_rows, int ld, const int32_t *row_idx,
                                                     const int32_t *src_valid_len, const int32_t *tgt, int ld_tgt,
                                                     const int32_t *tgt_valid_len, int batch, int steps, int tgt_len, float *loss,
                                                     float *logits_out) {
  TN_REQUIRE(t && table && row_idx && src_valid_len && tgt && tgt_valid_len && loss, "tn_gnmt_trainer_forward_backward_rows: null argument");
  TN_REQUIRE(n_rows >= 1 && ld >= t->F, "tn_gnmt_trainer_forward_backward_rows: needs n_rows >= 1 and ld >= the handle's input size");
  const SrcRows rows{table, n_rows, ld, row_idx};
  return trainer_step(t, nullptr, &rows, src_valid_len, tgt, ld_tgt, tgt_valid_len, batch, steps, tgt_len, loss, logits_out, nullptr, 0);
}

static int trainer_step(tn_gnmt_trainer *t, const float *src, const SrcRows *rows, const int32_t *src_valid_len, const int32_t *tgt, int ld,
                        const int32_t *tgt_valid_len, int batch, int steps, int tgt_len, float *loss, float *logits_out, float *dsrc, int ldd) {
  TN_REQUIRE(batch > 0 && batch <= t->maxB && steps > 0 && steps <= t->maxT && tgt_len >= 2 && tgt_len - 1 <= t->maxL && ld >= tgt_len,
             "tn_gnmt_trainer_forward_backward: batch / source steps / target length exceed the handle");
  TN_REQUIRE(!dsrc || ldd >= t->F, "gnmt_trainer_step: the source gradient's row stride is below input_size");
  TN_ON_DEVICE(t->ctx->device);
  hipStream_t s = t->ctx->stream;
  const int B = batch, T = steps, L = tgt_len - 1, H = t->H, E = t->E, V = t->V, G = t->G, GH = G * H, NL = t->NL;
  const int K0 = E + 2 * H, K1 = 3 * H;
  const int BT = B * T, LB = L * B;
  const bool lstm = G == 4;
  TN_REQUIRE(att_split(T, H, kStepLdsMax) > 0 && att_bwd_lds_bytes(T, H) <= kStepLdsMax,
             "tn_gnmt_trainer: 3 * max(hidden, source length) floats exceed 152 KiB of LDS");
  float *w = t->w, *g = t->g;
  const float *nul = nullptr;
  // ---------------- forward: encoder (gnmt.py:136-160) ----------------
  TN_HIP_CHECK(hipMemcpyAsync(t->vl, src_valid_len, sizeof(int32_t) * B, hipMemcpyDeviceToDevice, s));
  TN_TRY(launch_trn_dec_len(tgt_valid_len, t->tvl, B, s));
  const bool drop = t->drop_p > 0.f;
  const unsigned long long key = drop ? t->drop_seed * 0x2545F4914F6CDD1Dull + (++t->drop_count) * 0xD1342543DE82EF95ull : 0ull;
  std::vector<const float *> xin(NL + 1);     // layer i reads xin[i]; xin[NL] = the memory
  xin[0] = src;
  for (int i = 0; i < NL; ++i) {
    TrnEnc &e = t->enc[i];
    const int DG = e.D * GH;
    if (i == 0 && rows)
      TN_TRY(launch_linear_f32_padrows(rows->table, rows->ld, rows->idx, rows->n_rows, w + e.o_wi, e.in, w + e.o_bi, e.gi, DG, BT, DG, e.in, 0, s));
    else
      TN_TRY(launch_linear_f32(xin[i], e.in, w + e.o_wi, e.in, w + e.o_bi, e.gi, DG, BT, DG, e.in, 0, s));
    TN_HIP_CHECK(hipMemsetAsync(e.seq, 0, sizeof(float) * (size_t)BT * e.out, s));
    TN_TRY(launch_rnn_recurrent(G, e.gi, DG, e.whT, w + e.o_bh, t->vl, e.seq, e.out, e.hl, lstm ? e.cl : nullptr, B, T, H, e.D, s, e.sav));
    // dropout on the layer's output (the states are not dropped), then the residual connection (gnmt.py:152-157)
    const long no = (long)BT * e.out;
    if (drop) TN_TRY(launch_trn_dropout_mask(e.M, no, t->drop_p, key ^ (0x1111ull * (i + 1)), s));
    if (drop || e.res) {
      TN_TRY(launch_mul_add(e.seq, drop ? e.M : nul, e.res ? xin[i] : nul, e.xn, no, s));
      xin[i + 1] = e.xn;
    } else {
      xin[i + 1] = e.seq;
    }
  }
  const float *mem = xin[NL];
  TN_TRY(launch_linear_f32(mem, H, w + t->o_wk, H, nullptr, t->keyproj, H, BT, H, H, 0, s));
  TN_TRY(launch_transpose_bth(t->keyproj, t->keyprojT, B, T, H, s));
  // the decoder layer j starts from encoder layer j's final state: the BACKWARD direction's for a bidirectional layer (gnmt.py:146-150)
  auto h_init = [&](int j) { return (const float *)(t->enc[j].hl + (size_t)(t->enc[j].D - 1) * B * H); };
  auto c_init = [&](int j) { return (const float *)(t->enc[j].cl + (size_t)(t->enc[j].D - 1) * B * H); };
  // ---------------- forward: decoder steps (gnmt.py:369-404) ----------------
  if (drop)
    for (int j = 1; j < NL; ++j)
      TN_TRY(launch_trn_dropout_mask(t->dec[j].M, (long)LB * H, t->drop_p, key ^ (0x3333ull * j), s));
  TrnDec &d0 = t->dec[0], &d1 = t->dec[1];
  DecAttentionArgs at;
  at.ldh = K0; at.lstm = lstm; at.hn = t->h0tmp; at.ldx1 = K1; at.kpT = t->keyprojT; at.mem = mem; at.valid_len = t->vl; at.ctx = t->ctxtmp;
  at.R = B; at.T = T; at.H = H;
  for (int i = 0; i < L; ++i) {
    const size_t so = (size_t)i * B, sp = (size_t)(i - 1) * B;
    float *X0 = d0.X + so * K0, *X1 = d1.X + so * K1;
    const float *X1p = d1.X + sp * K1;
    // step inputs, strided sources: x0 = [embed(tok), ctx_prev | 0, h0_prev], x1[:, 2H:3H] = h1_prev
    TN_TRY(launch_dec_prep(w + t->o_emb, tgt, ld, i, i ? X1p + H : nul, K1, i ? X1p : h_init(0), i ? K1 : H, i ? d1.Hs + sp * H : h_init(1), H, nul,
                           nul, X0, X1, K1, nullptr, nullptr, 1, B, H, E, s));
    for (int j = 2; j < NL; ++j)
      TN_TRY(launch_mul_add_rows(i ? t->dec[j].Hs + sp * H : h_init(j), H, nul, nul, 0, t->dec[j].X + so * K1 + 2 * H, K1, B, H, s));
    TN_TRY(launch_linear_f32_lat(X0, K0, d0.wc, K0, d0.bc, d0.G + so * 4 * H, 4 * H, B, 4 * H, K0, s));
    at.g0 = d0.G + so * 4 * H; at.hprev = X0 + E + H; at.cprev = !lstm ? nul : i ? d0.C + sp * H : c_init(0);
    at.cn = lstm ? d0.C + so * H : nullptr; at.x1 = X1; at.wsave = t->AW + so * T;
    TN_TRY(launch_dec_attention(at, s));
    for (int j = 1; j < NL; ++j) {
      TrnDec &d = t->dec[j];
      const bool top = j == NL - 1;
      float *Xj = d.X + so * K1;
      TN_TRY(launch_linear_f32_lat(Xj, K1, d.wc, K1, d.bc, d.G + so * 4 * H, 4 * H, B, 4 * H, K1, s));
      const float *cp = !lstm ? nul : i ? (const float *)(d.C + sp * H) : c_init(j);
      float *outp = top ? t->Out + so * H : t->dec[j + 1].X + so * K1;
      TN_TRY(launch_dec_cell(d.G + so * 4 * H, Xj, lstm, cp, d.Hs + so * H, lstm ? d.C + so * H : nullptr, drop ? d.M + so * H : nul, t->residual,
                             outp, top ? H : K1, top ? nullptr : outp + H, B, H, s));
    }
    TN_TRY(launch_linear_f32_lat(t->Out + so * H, H, w + t->o_wp, H, w + t->o_bp, t->logits + (size_t)i * V, L * V, B, V, H, s));
  }
  // ---------------- loss and its gradient ----------------
  TN_TRY(launch_trn_ce_bwd(t->logits, tgt + 1, ld, t->tvl, B, L, V, t->dlog, t->lossrows, s));
  TN_TRY(launch_colsum_f32(t->lossrows, 1, LB, 1, loss, s));
  if (logits_out) TN_HIP_CHECK(hipMemcpyAsync(logits_out, t->logits, sizeof(float) * (size_t)LB * V, hipMemcpyDeviceToDevice, s));
  // ---------------- backward: projection ----------------
  TN_TRY(launch_linear_f32(t->dlog, V, t->wpT, V, nullptr, t->dOut, H, LB, H, V, 0, s));
  TN_TRY(launch_gemm_tn_f32(t->dlog, V, t->Out, H, g + t->o_wp, H, V, H, LB, s));
  TN_TRY(launch_colsum_f32(t->dlog, V, LB, V, g + t->o_bp, s));
  float *dmem = t->enc[NL - 1].dxn;      // (written, with t->dkp, by trn_att_outer_kernel after the loop)
  // ---------------- backward: decoder steps, last to first ----------------
  for (int i = L - 1; i >= 0; --i) {
    const bool last = i == L - 1;
    const size_t so = (size_t)i * B, sp = (size_t)(i - 1) * B, sn = (size_t)(i + 1) * B;
    // d (output of layer j), walking down from the rows the projection read: pointer + row stride
    const float *dcur = t->dOut + so * H;
    int ldcur = H;
    float *pingpong[2] = {t->tmpA, t->tmpB};
    int pp = 0;
    for (int j = NL - 1; j >= 1; --j) {
      TrnDec &d = t->dec[j];
      const float *Xj = d.X + so * K1, *Gj = d.G + so * 4 * H;
      float *dGj = d.dG + so * 4 * H, *dXj = d.dX + so * K1;
      const float *dXjn = d.dX + sn * K1;
      // through the dropout mask to the cell's h
      const float *dh = dcur;
      int ldh = ldcur;
      if (drop) {
        TN_TRY(launch_mul_add_rows(dcur, ldcur, d.M + so * H, nul, 0, t->tmpM, H, B, H, s));
        dh = t->tmpM; ldh = H;
      }
      if (lstm)
        TN_TRY(launch_trn_lstm_bwd(Gj, i ? d.C + sp * H : c_init(j), d.C + so * H, dh, ldh, last ? nul : d.dhz, H, last ? nul : dXjn + 2 * H, K1, nul,
                                   0, last ? nul : d.dcz, dGj, d.dhz, d.dcz, B, H, s));
      else
        TN_TRY(launch_trn_gru_bwd(Gj, Xj + 2 * H, K1, dh, ldh, last ? nul : d.dhz, H, last ? nul : dXjn + 2 * H, K1, nul, 0, dGj, d.dhz, B, H, s));
      TN_TRY(launch_linear_f32_lat(dGj, 4 * H, d.wcT, 4 * H, nullptr, dXj, K1, B, K1, 4 * H, s));
      // d (the layer's input) = its column block of dX (+ the residual path)
      if (t->residual) {
        float *dst = pingpong[pp]; pp ^= 1;
        TN_TRY(launch_mul_add_rows(dXj, K1, nul, dcur, ldcur, dst, H, B, H, s));
        dcur = dst; ldcur = H;
      } else {
        dcur = dXj; ldcur = K1;
      }
    }
    // attention: d ctx = the attention columns of every layer's dX at this step + the first cell's at the next step
    const float *datt = t->dec[1].dX + so * K1 + H;
    int ldatt = K1;
    if (NL > 2) {
      TN_TRY(launch_mul_add_rows(datt, K1, nul, t->dec[2].dX + so * K1 + H, K1, t->tmpAtt, H, B, H, s));
      for (int j = 3; j < NL; ++j) TN_TRY(launch_mul_add_rows(t->tmpAtt, H, nul, t->dec[j].dX + so * K1 + H, K1, t->tmpAtt, H, B, H, s));
      datt = t->tmpAtt; ldatt = H;
    }
    const float *dX0n = d0.dX + sn * K0;
    TN_TRY(launch_trn_att_bwd(t->AW + so * T, mem, t->keyproj, datt, ldatt, last ? nul : dX0n + E, K0, t->vl, t->DS + so * T, t->DCTX + so * H, t->dq,
                              B, T, H, s));
    // first cell: d h0 = d (layer 1's input) + the query's gradient + the recurrent paths
    const float *X0 = d0.X + so * K0, *G0 = d0.G + so * 4 * H;
    float *dG0 = d0.dG + so * 4 * H, *dX0 = d0.dX + so * K0;
    if (lstm)
      TN_TRY(launch_trn_lstm_bwd(G0, i ? d0.C + sp * H : c_init(0), d0.C + so * H, dcur, ldcur, t->dq, H, last ? nul : d0.dhz, H,
                                 last ? nul : dX0n + E + H, K0, last ? nul : d0.dcz, dG0, d0.dhz, d0.dcz, B, H, s));
    else
      TN_TRY(launch_trn_gru_bwd(G0, X0 + E + H, K0, dcur, ldcur, t->dq, H, last ? nul : d0.dhz, H, last ? nul : dX0n + E + H, K0, dG0, d0.dhz, B, H, s));
    TN_TRY(launch_linear_f32_lat(dG0, 4 * H, d0.wcT, 4 * H, nullptr, dX0, K0, B, K0, 4 * H, s));
  }
  // gradients reaching the encoder's final states: decoder layer j's initial state is encoder layer j's (backward direction of a bi layer)
  for (int j = 0; j < NL; ++j) {
    TrnEnc &e = t->enc[j];
    TrnDec &d = t->dec[j];
    if (e.D == 2) {
      TN_HIP_CHECK(hipMemsetAsync(e.dhl, 0, sizeof(float) * (size_t)B * H, s));
      if (lstm) TN_HIP_CHECK(hipMemsetAsync(e.dcl, 0, sizeof(float) * (size_t)B * H, s));
    }
    const size_t off = (size_t)(e.D - 1) * B * H;
    TN_TRY(launch_mul_add_rows(d.dhz, H, nul, d.dX + (j ? 2 * H : E + H), d.K, e.dhl + off, H, B, H, s));
    if (lstm) TN_HIP_CHECK(hipMemcpyAsync(e.dcl + off, d.dcz, sizeof(float) * (size_t)B * H, hipMemcpyDeviceToDevice, s));
  }
  // ---------------- backward: decoder weights, attention key projection, embedding ----------------
  for (int j = 0; j < NL; ++j) {
    TrnDec &d = t->dec[j];
    TN_TRY(launch_gemm_tn_f32(d.dG, 4 * H, d.X, d.K, d.dW, d.K, 4 * H, d.K, LB, s));
    TN_TRY(launch_colsum_f32(d.dG, 4 * H, LB, 4 * H, d.db, s));
    TN_TRY(launch_trn_unstack(d.dW, d.db, d.in, H, lstm, g + d.o_wi, g + d.o_wh, g + d.o_bi, g + d.o_bh, s));
  }
  TN_TRY(launch_trn_att_outer(t->AW, t->DS, t->DCTX, d1.X, K1, dmem, t->dkp, L, B, T, H, s));
  TN_TRY(launch_gemm_tn_f32(t->dkp, H, mem, H, g + t->o_wk, H, H, H, BT, s));
  TN_TRY(launch_linear_f32(t->dkp, H, t->wkT, H, nullptr, dmem, H, BT, H, H, 1, s));
  TN_TRY(launch_trn_emb_grad(d0.dX, K0, tgt, ld, B, L, E, V, g + t->o_emb, s));
  // ---------------- backward: encoder, last layer to first ----------------
  for (int i = NL - 1; i >= 0; --i) {
    TrnEnc &e = t->enc[i];
    const int DG = e.D * GH;
    const long no = (long)BT * e.out;
    // e.dxn = d (what the next layer read); through the dropout mask to the recurrence's outputs
    const float *dseq = e.dxn;
    if (drop) {
      TN_TRY(launch_mul_add(e.dxn, e.M, nul, e.dseq, no, s));
      dseq = e.dseq;
    }
    TN_HIP_CHECK(hipMemsetAsync(e.dgi, 0, sizeof(float) * (size_t)BT * DG, s));
    TN_HIP_CHECK(hipMemsetAsync(e.dgh, 0, sizeof(float) * (size_t)BT * DG, s));
    TN_HIP_CHECK(hipMemsetAsync(e.hp, 0, sizeof(float) * (size_t)e.D * BT * H, s));
    TN_TRY(launch_rnn_bptt(G, e.seq, e.sav, dseq, w + e.o_wh, e.dgi, e.dgh, e.hp, B, T, H, s, e.D, t->vl, e.dhl, e.dcl));
    const float *dgh = lstm ? e.dgi : e.dgh;      // LSTM: one pre-activation gradient feeds both branches
    if (i == 0 && rows)       // dW_ih = dGI^T src, src gathered: one slice, as the call below (no workspace)
      TN_TRY(launch_gemm_tn_f32_padrows(e.dgi, DG, rows->table, rows->ld, rows->idx, rows->n_rows, g + e.o_wi, e.in, DG, e.in, BT, s));
    else
      TN_TRY(launch_gemm_tn_f32(e.dgi, DG, xin[i], e.in, g + e.o_wi, e.in, DG, e.in, BT, s));
    TN_TRY(launch_colsum_f32(e.dgi, DG, BT, DG, g + e.o_bi, s));
    for (int d = 0; d < e.D; ++d)
      TN_TRY(launch_gemm_tn_f32(dgh + (size_t)d * GH, DG, e.hp + (size_t)d * BT * H, H, g + e.o_wh + (long)d * GH * H, H, GH, H, BT, s));
    TN_TRY(launch_colsum_f32(dgh, DG, BT, DG, g + e.o_bh, s));
    if (i > 0) {       // d (this layer's input) = d (the layer below's xn): through the input weights (+ the residual path)
      TrnEnc &below = t->enc[i - 1];
      TN_TRY(launch_linear_f32(e.dgi, DG, e.wiT, DG, nullptr, below.dxn, e.in, BT, e.in, DG, 0, s));
      if (e.res) TN_TRY(launch_mul_add(below.dxn, nul, e.dxn, below.dxn, (long)BT * e.in, s));
    } else if (dsrc) {
      // d src = dGI W_ih: dgi (BT, D GH) and W_ih (D GH, F) as the trainer keeps them (the directions stacked, row-major) are
      // gemm_nn's operands as they stand.  This is the whole gradient: src reaches the loss through layer 0's input product alone -
      // a residual connection adds a layer's input only for layers i > num_bi_layers >= 0 (gnmt.py:155-157), so never layer 0's,
      // and dropout acts on layer outputs (gnmt.py:152).  Rows at or past the valid length: the recurrence backward does not
      // write their dgi, which the memset above left at 0, so their product is exactly 0.
      TN_TRY(launch_gemm_nn_f32(e.dgi, DG, w + e.o_wi, e.in, dsrc, ldd, BT, e.in, DG, 0, s));
    }
  }
  return TN_OK;
}

// dropout rate of the encoder / decoder layers (train_gnmt.py --dropout, default 0.2 there; 0 here until set) and the
// seed of the counter-based mask generator.  MXNet's own random stream cannot be reproduced: masks differ from the
// reference's, their distribution and placement do not.
extern "C" int tn_gnmt_trainer_set_dropout(tn_gnmt_trainer *t, float p, uint64_t seed) {
  TN_REQUIRE(t, "tn_gnmt_trainer_set_dropout: null handle");
  TN_REQUIRE(p >= 0.f && p < 1.f, "tn_gnmt_trainer_set_dropout: rate must be in [0, 1)");
  t->drop_p = p; t->drop_seed = seed; t->drop_count = 0;
  return TN_OK;
}
// the masks of the last forward_backward (device pointers) - test hook.  which = 0 .. num_layers - 1: encoder layer's (B*T, D H);
// num_layers + j, j = 1 .. num_layers - 1: decoder layer j's (L*B, H) step-major
extern "C" int tn_gnmt_trainer_dropout_mask(tn_gnmt_trainer *t, int which, float **mask) {
  TN_REQUIRE(t && mask, "tn_gnmt_trainer_dropout_mask: null argument");
  TN_REQUIRE(which >= 0 && which < 2 * t->NL && which != t->NL, "tn_gnmt_trainer_dropout_mask: no such mask");
  *mask = which < t->NL ? t->enc[which].M : t->dec[which - t->NL].M;
  return TN_OK;
}
// (the two-layer form of round 2: encoder layers 0 / 1 and the top decoder layer)
extern "C" int tn_gnmt_trainer_dropout_masks(tn_gnmt_trainer *t, float **m_enc0, float **m_enc1, float **m_dec) {
  TN_REQUIRE(t && m_enc0 && m_enc1 && m_dec, "tn_gnmt_trainer_dropout_masks: null argument");
  *m_enc0 = t->enc[0].M; *m_enc1 = t->enc[1].M; *m_dec = t->dec[t->NL - 1].M;
  return TN_OK;
}

extern "C" int tn_gnmt_trainer_buffers(tn_gnmt_trainer *t, float **params_dev, float **grads_dev, int64_t *numel) {
  return train_buffers("tn_gnmt_trainer_buffers", t, params_dev, grads_dev, numel);
}

// gluon.Trainer(params, 'adam', {'learning_rate': lr}).step(1) (train_gnmt.py:310,337): MXNet Adam, beta1 0.9, beta2 0.999,
// epsilon 1e-8, no weight decay, rescale_grad 1; no clipping unless tn_gnmt_trainer_set_clip switched it on (the reference defines
// --clip, train_gnmt.py:97-98, and never applies it), then gluon.utils.clip_global_norm [EXT] ahead of the update
extern "C" int tn_gnmt_trainer_adam_step(tn_gnmt_trainer *t, float lr, float beta1, float beta2, float epsilon) {
  TN_REQUIRE(t, "tn_gnmt_trainer_adam_step: null handle");
  if (!t->clip.on()) return gnmt_trainer_adam(t, lr, beta1, beta2, epsilon, t->step + 1, nullptr);
  TN_ON_DEVICE(t->ctx->device);
  if (int rc = t->clip.reduce(t->ctx, t->g, t->n, nullptr, 0, 1.f)) return rc;
  return gnmt_trainer_adam(t, lr, beta1, beta2, epsilon, t->step + 1, t->clip.scale());
}
extern "C" int tn_gnmt_trainer_set_clip(tn_gnmt_trainer *t, float max_norm) {
  TN_REQUIRE(t, "tn_gnmt_trainer_set_clip: null handle");
  return t->clip.set("tn_gnmt_trainer_set_clip", t->ctx, max_norm);
}
extern "C" int tn_gnmt_trainer_clip_stats(tn_gnmt_trainer *t, float *norm, float *scale, int64_t *clipped_steps) {
  TN_REQUIRE(t, "tn_gnmt_trainer_clip_stats: null handle");
  return t->clip.stats("tn_gnmt_trainer_clip_stats", t->ctx, norm, scale, clipped_steps);
}
// the update for the step-th time (train.h): the frame-mode handle counts once for the backbone and the captioner
int gnmt_trainer_adam(tn_gnmt_trainer *t, float lr, float beta1, float beta2, float epsilon, long step, const float *scale) {
  TN_ON_DEVICE(t->ctx->device);
  t->step = step;
  if (int rc = launch_adam(t->w, t->g, t->am, t->av, t->n, lr, beta1, beta2, epsilon, step, t->ctx->stream, scale)) return rc;
  return trainer_refresh(t);
}

extern "C" int tn_gnmt_trainer_read_param(tn_gnmt_trainer *t, const char *name, int gradient, float *out_host, int64_t capacity,
                                          int64_t *numel) {
  return train_read_param("tn_gnmt_trainer_read_param", t, name, gradient, out_host, capacity, numel);
}

extern "C" int tn_gnmt_trainer_destroy(tn_gnmt_trainer *t) {
  if (!t) return TN_OK;
  TnDeviceGuard tn_dg_(t->ctx->device);
  (void)hipStreamSynchronize(t->ctx->stream);
  t->clip.release();
  t->pool.release();
  delete t;
  return TN_OK;
}
