// GNMT captioner, inference, fp32 throughout:
//   encoder      GNMTEncoder.forward, reference models/captioning/gnmt.py:136-160
//                (bi-GRU with valid_length + uni-GRU, reusing the tn_birnn kernels)
//   init state   GNMTDecoder.init_state_from_encoder, gnmt.py:224-252
//   decode step  GNMTDecoder.hybrid_forward, gnmt.py:345-404, behind NMTModel.decode_step
//                [EXT]: tgt_embed -> GRUCell0([emb, att]) -> scaled-Luong attention ->
//                GRUCell1([h0, ctx]) -> tgt_proj -> log_softmax (utils/translation.py:51-53)
//   beam search  gluonnlp BeamSearchSampler/Scorer [EXT] as driven by
//                BeamSearchTranslator.translate, utils/translation.py:55-82
// One decode step = four launches, shared by the beam search and by teacher forcing (decode_seq): a stacked-gate
// GEMM per cell (linear.hip), dec_attention_kernel (cell-0 gates + attention) and dec_beam_kernel (cell-1 gates +
// projection + beam update + the next step's gathered inputs) resp. dec_cell_kernel + the projection GEMM (the kernels and
// their launchers: gnmt_kernels.hip; the training handle: captioner_train.hip).  The whole token loop is enqueued on the stream with no per-step host sync; the host
// looks at a device flag every 16 steps only to stop early once every beam has finished.
// On request (tn_gnmt_decode_seq_attention / tn_gnmt_beam_search_attention, gnmt.py:302-303,402-403) the steps' attention weights
// are returned too: teacher forcing stores them in place, the beam search keeps every step's rows in a history of
// 4 * max_length * max_batch * beam * max_src_len bytes (61.4 MB for 150 x 32 x 5 x 640; allocated by the first search that asks,
// never otherwise) and gathers the final hypotheses' rows along their back-pointers (beam_att_rows_kernel, beam_att_gather_kernel).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "api_internal.h"
#include "gnmt_kernels.h"
#include "linear.h"
#include "rnn.h"
#include "train.h"

constexpr int kGemmPitchPad = 16;   // floats; measured at config C5: 0 / 32 / 64 / 96: 44.2 us per step, 16 / 48 / 80: 42.2

// a decoder cell between the first and the last one (num_layers > 2)
struct GnmtMid { float *w, *b, *sx, *g, *hn, *cn, *ccur; };

struct tn_gnmt {
  tn_ctx *ctx;
  DevPool pool;
  // encoder: num_bi_layers bidirectional layers (F | 2H -> 2H), then uni-directional ones (2H | H -> H); gnmt.py:84-111
  std::vector<tn_birnn *> enc;
  int NL, NBI;
  bool residual;            // use_residual (gnmt.py:155-157, 394-395)
  std::vector<float *> hl, cl;   // final states per encoder layer (bi: [fwd, bwd]); the decoder layer i starts from layer i's
  float *seqB;              // second sequence buffer (layers ping-pong between seq0 and seqB; the last one writes mem)
  std::vector<GnmtMid> mid; // decoder layers 1 .. NL-2
  float *hstate;            // last decoder layer's state when use_residual (the LDS copy then holds h + input)
  int32_t *parent;          // parent beam per row (for the states of `mid`)
  int F, H, E, V, maxB, maxT, beam, maxL;
  float *wk, *wp, *bp, *emb;
  // per-call workspace
  int G;                   // gates per cell: 3 GRU, 4 LSTM
  float *seq0, *mem, *keyproj;
  int32_t *vl;
  float *scores;
  int32_t *alive, *vlen, *tok, *samples[2], *flag;
  // fused beam-search step: stacked [i2h | h2h] weights (4H rows each), transposed projection, step buffers
  float *w0c, *b0c, *w1c, *b1c, *wpT, *bpp;   // (wpT, bpp: Wp^T and its bias with rows / length padded to a multiple of 4)
  float *sx0, *sx1, *g0, *g1, *h0n, *ctxn, *c0n, *c0cur, *c1cur, *keyprojT, *h1n, *c1n;
  // two decoder layers: the first cell's gate GEMM leaves the step's critical path (dec_beam_kernel, `tok_out`):
  // w1x (4H, 3H) = the first cell's columns of h0 and ctx in the order of x1 = [h0, ctx, h1_prev] (the last H columns unused),
  // b1x = b0, ew (V, 4H) = embedding . first cell's embedding columns (made on the first search), p0 (R, 4H) the [h0, ctx]
  // share of the next step's pre-activations, h0n2 / c0n2 the second buffers of the first cell's states (a step reads the
  // previous step's by parent row while it writes its own)
  float *w1x, *b1x, *ew, *p0, *h0n2, *c0n2, *w1cp, *sx1p, *w1k4;
  int K1p;                 // pitch of w1cp / w1x / sx1p, see kGemmPitchPad
  bool ew_ready;
  int32_t *bp_par, *bp_word;   // (maxL, R) back-pointers of the search
  // attention weights on request (tn_gnmt_beam_search_attention): the steps' rows (max_length, R, maxT) and the final
  // hypotheses' ancestor rows (R, max_length); null until a search asks for the weights (beam_att_rows_kernel)
  float *att_hist;
  int32_t *att_rows;
  int B, T;
};

extern "C" int tn_gnmt_create_ex(tn_ctx *ctx, const tn_param *params, int n_params, const char *prefix_c, int cell_kind,
                                 int input_size, int hidden, int embed, int vocab, int num_layers, int num_bi_layers,
                                 int max_batch, int max_src_len, int beam, int max_length, int flags, tn_gnmt **out) {
  TN_REQUIRE(ctx && params && prefix_c && out, "tn_gnmt_create: null argument");
  TN_REQUIRE(cell_kind == TN_RNN_GRU || cell_kind == TN_RNN_LSTM, "tn_gnmt_create: cell_type must be 'gru' or 'lstm'");
  TN_REQUIRE((flags & ~TN_GNMT_USE_RESIDUAL) == 0, "tn_gnmt_create_ex: unknown flag");
  // gnmt.py:78-80 asserts num_bi_layers <= num_layers; with num_bi_layers == num_layers the memory is 2H wide and gluonnlp's
  // Luong-style attention (key width = units = H) refuses it [EXT]; a one-layer decoder has no cell behind the attention
  TN_REQUIRE(num_layers >= 2 && num_layers <= 8 && num_bi_layers >= 0 && num_bi_layers < num_layers,
             "tn_gnmt_create: need 2 <= num_layers <= 8 and 0 <= num_bi_layers < num_layers");
  TN_REQUIRE(beam >= 1 && beam <= 16 && vocab >= beam && max_length >= 1, "tn_gnmt_create: bad beam/vocab/max_length");
  TN_REQUIRE(input_size > 0 && hidden > 0 && hidden % 4 == 0 && embed > 0 && max_batch > 0 && max_src_len > 0,
             "tn_gnmt_create: bad shape");
  TN_ON_DEVICE(ctx->device);
  const std::string pre(prefix_c);
  const ParamMap pm(params, n_params);
  tn_gnmt *g = new tn_gnmt();   // value-initialised: every pointer member starts null
  g->ctx = ctx; g->F = input_size; g->H = hidden; g->E = embed; g->V = vocab; g->maxB = max_batch; g->maxT = max_src_len;
  g->beam = beam; g->maxL = max_length + 2; g->G = cell_kind == TN_RNN_GRU ? 3 : 4;
  g->NL = num_layers; g->NBI = num_bi_layers; g->residual = (flags & TN_GNMT_USE_RESIDUAL) != 0;
  auto fail = [&](int code) { g->pool.release(); for (tn_birnn *e : g->enc) tn_birnn_destroy(e); delete g; return code; };
  const char *sfx[4] = {"i2h_weight", "h2h_weight", "i2h_bias", "h2h_bias"};
  const int H = hidden, G3 = g->G * hidden;   // (G3: gates * hidden, 3H or 4H)
  // encoder layers: "<pre>enc_rnn{i}_{l,r}_*" (bidirectional) / "<pre>enc_rnn{i}_*" -> the "{l,r}0_*" names of tn_birnn
  for (int i = 0, fin = input_size; i < num_layers; ++i) {
    const bool bi = i < num_bi_layers;
    std::vector<tn_param> pl;
    std::vector<std::string> names;
    names.reserve(8);
    for (int d = 0; d < (bi ? 2 : 1); ++d)
      for (int k = 0; k < 4; ++k) {
        const std::string src = pre + "enc_rnn" + std::to_string(i) + "_" + (bi ? (d ? "r_" : "l_") : "") + sfx[k];
        const int64_t n = k == 0 ? (int64_t)G3 * fin : k == 1 ? (int64_t)G3 * H : G3;
        const float *v = pm.get(src, n);
        if (!v) return fail(TN_ERR_MISSING);
        names.push_back(std::string(d ? "r0_" : "l0_") + sfx[k]);
        pl.push_back(tn_param{nullptr, v, n});
      }
    for (size_t k = 0; k < pl.size(); ++k) pl[k].name = names[k].c_str();
    tn_birnn *e = nullptr;
    const int rc = tn_birnn_create(ctx, (tn_rnn_kind)cell_kind, fin, H, pl.data(), (int)pl.size(), "", bi ? 1 : 0, max_batch * max_src_len, &e);
    if (rc) return fail(rc);
    g->enc.push_back(e);
    fin = bi ? 2 * H : H;
  }
  // decoder
  const float *a;
#define UP(dst, name, n) do { a = pm.get(pre + name, (int64_t)(n)); if (!a) return fail(TN_ERR_MISSING); dst = g->pool.upload(a, (size_t)(n)); } while (0)
  UP(g->wk, "dec_attention_key_weight", (int64_t)H * H);
  UP(g->wp, "tgt_proj_weight", (int64_t)vocab * H); UP(g->bp, "tgt_proj_bias", vocab);
  UP(g->emb, "tgt_embed_weight", (int64_t)vocab * embed);
#undef UP
  {
    // one GEMM per decoder cell: rows of the stacked matrix = 4H gate columns over [cell input | h_prev].
    // LSTM: [Wi | Wh], bias bi + bh.  GRU: r and z likewise; the candidate keeps its two branches apart
    // (n = tanh(n_i2h + r * n_h2h)): rows 2H..3H = [Wi_n | 0], rows 3H..4H = [0 | Wh_n].
    std::vector<float> last_w, last_b;      // host copies of the matrix stack() made last
    auto stack = [&](const std::string &cell, int in_dim, float **w_out, float **b_out) -> bool {
      const float *wi = pm.get(pre + cell + "i2h_weight", (int64_t)G3 * in_dim), *wh = pm.get(pre + cell + "h2h_weight", (int64_t)G3 * H);
      const float *bi = pm.get(pre + cell + "i2h_bias", G3), *bh = pm.get(pre + cell + "h2h_bias", G3);
      if (!wi || !wh || !bi || !bh) return false;
      const int Kc = in_dim + H;
      std::vector<float> w((size_t)4 * H * Kc, 0.f), bv(4 * H, 0.f);
      for (int row = 0; row < 4 * H; ++row) {
        float *d = &w[(size_t)row * Kc];
        if (g->G == 4 || row < 2 * H) {
          memcpy(d, wi + (size_t)row * in_dim, sizeof(float) * in_dim);
          memcpy(d + in_dim, wh + (size_t)row * H, sizeof(float) * H);
          bv[row] = bi[row] + bh[row];
        } else if (row < 3 * H) {
          memcpy(d, wi + (size_t)row * in_dim, sizeof(float) * in_dim);
          bv[row] = bi[row];
        } else {
          memcpy(d + in_dim, wh + (size_t)(row - H) * H, sizeof(float) * H);
          bv[row] = bh[row - H];
        }
      }
      *w_out = g->pool.upload(w.data(), w.size());
      *b_out = g->pool.upload(bv.data(), bv.size());
      last_w.swap(w); last_b.swap(bv);
      return true;
    };
    if (!stack("dec_rnn0_", embed + H, &g->w0c, &g->b0c)) return fail(TN_ERR_MISSING);
    std::vector<float> w0, b0;
    w0.swap(last_w); b0.swap(last_b);
    if (!stack("dec_rnn" + std::to_string(num_layers - 1) + "_", 2 * H, &g->w1c, &g->b1c)) return fail(TN_ERR_MISSING);
    if (num_layers == 2) {
      const int K0 = embed + 2 * H, K1 = 3 * H;
      // the step GEMMs read 16 operand rows per load instruction: with rows 3H floats apart (3 KiB at H = 256) the sixteen
      // lines of an instruction fall into a quarter of the L2 channels; the rows of the beam search's operands get a pitch
      // that spreads them (tuning: TN_GNMT_PAD=<floats>)
      const char *pe = getenv("TN_GNMT_PAD");
      const int K1p = K1 + (((pe ? std::max(0, atoi(pe)) : kGemmPitchPad) + 3) & ~3);      // (rows stay 16-byte aligned)
      g->K1p = K1p;
      const std::vector<float> &w1 = last_w;
      std::vector<float> w1p((size_t)4 * H * K1p, 0.f);
      for (int row = 0; row < 4 * H; ++row) memcpy(&w1p[(size_t)row * K1p], &w1[(size_t)row * K1], sizeof(float) * K1);
      g->w1cp = g->pool.upload(w1p.data(), w1p.size());
      g->w1k4 = g->pool.upload(pack_wk4(w1.data(), 4 * H, K1));      // the same weights k-group-major for the step's gate GEMM
      g->sx1p = g->pool.alloc<float>((size_t)max_batch * beam * K1p);      // (k-group-major in the beam search: K1 x rows floats)
      std::vector<float> wx((size_t)4 * H * K1p, 0.f);
      for (int row = 0; row < 4 * H; ++row) {
        float *d = &wx[(size_t)row * K1p];
        const float *sw = &w0[(size_t)row * K0];
        memcpy(d, sw + embed + H, sizeof(float) * H);        // x1[:, 0:H] = h0   <- x0[:, E+H:]
        memcpy(d + H, sw + embed, sizeof(float) * H);        // x1[:, H:2H] = ctx <- x0[:, E:E+H]
      }
      g->w1x = g->pool.upload(wx.data(), wx.size());
      g->b1x = g->pool.upload(b0.data(), b0.size());
      g->ew = g->pool.alloc<float>((size_t)vocab * 4 * H);
    }
    g->mid.resize(num_layers - 2);
    for (int i = 1; i + 1 < num_layers; ++i)
      if (!stack("dec_rnn" + std::to_string(i) + "_", 2 * H, &g->mid[i - 1].w, &g->mid[i - 1].b)) return fail(TN_ERR_MISSING);
    const float *wp = pm.get(pre + "tgt_proj_weight", (int64_t)vocab * H);
    const float *bpv = pm.get(pre + "tgt_proj_bias", vocab);
    std::vector<float> wt, bpad;
    pack_proj(wp, bpv, vocab, H, wt, bpad);
    g->wpT = g->pool.upload(wt.data(), wt.size());
    g->bpp = g->pool.upload(bpad.data(), bpad.size());
  }
  const size_t BT = (size_t)max_batch * max_src_len, R = (size_t)max_batch * beam;
  g->seq0 = g->pool.alloc<float>(BT * 2 * H); g->mem = g->pool.alloc<float>(BT * H); g->keyproj = g->pool.alloc<float>(BT * H);
  g->seqB = num_layers > 2 ? g->pool.alloc<float>(BT * 2 * H) : nullptr;
  for (int i = 0; i < num_layers; ++i) {
    g->hl.push_back(g->pool.alloc<float>(2 * (size_t)max_batch * H));
    g->cl.push_back(g->pool.alloc<float>(2 * (size_t)max_batch * H));
  }
  for (GnmtMid &m : g->mid) {
    m.sx = g->pool.alloc<float>(R * 3 * H); m.g = g->pool.alloc<float>(R * 4 * H);
    m.hn = g->pool.alloc<float>(R * H); m.cn = g->pool.alloc<float>(R * H); m.ccur = g->pool.alloc<float>(R * H);
  }
  g->hstate = g->residual ? g->pool.alloc<float>(R * H) : nullptr;
  g->parent = g->pool.alloc<int32_t>(R);
  g->vl = g->pool.alloc<int32_t>(max_batch);
  g->samples[0] = g->pool.alloc<int32_t>(R * g->maxL);
  g->bp_par = g->pool.alloc<int32_t>(R * g->maxL); g->bp_word = g->pool.alloc<int32_t>(R * g->maxL);
  g->scores = g->pool.alloc<float>(R); g->alive = g->pool.alloc<int32_t>(R); g->vlen = g->pool.alloc<int32_t>(R);
  g->tok = g->pool.alloc<int32_t>(R); g->flag = g->pool.alloc<int32_t>(1);
  g->h1n = g->pool.alloc<float>(R * H); g->c1n = g->pool.alloc<float>(R * H);
  g->sx0 = g->pool.alloc<float>(R * (embed + 2 * H)); g->sx1 = g->pool.alloc<float>(R * 3 * H);
  g->g0 = g->pool.alloc<float>(R * 4 * H); g->g1 = g->pool.alloc<float>(R * 4 * H);
  if (num_layers == 2) {
    g->p0 = g->pool.alloc<float>(R * 4 * H); g->h0n2 = g->pool.alloc<float>(R * H); g->c0n2 = g->pool.alloc<float>(R * H);
  }
  g->h0n = g->pool.alloc<float>(R * H); g->ctxn = g->pool.alloc<float>(R * H); g->c0n = g->pool.alloc<float>(R * H);
  g->c0cur = g->pool.alloc<float>(R * H); g->c1cur = g->pool.alloc<float>(R * H); g->keyprojT = g->pool.alloc<float>((size_t)max_batch * ((max_src_len + 3) & ~3) * H);
  if (g->pool.failed) { tn_set_error("device allocation failed"); return fail(TN_ERR_NOMEM); }
  *out = g;
  return TN_OK;
}
extern "C" int tn_gnmt_create(tn_ctx *ctx, const tn_param *params, int n_params, const char *prefix_c, int cell_kind,
                              int input_size, int hidden, int embed, int vocab, int num_layers, int num_bi_layers,
                              int max_batch, int max_src_len, int beam, int max_length, tn_gnmt **out) {
  return tn_gnmt_create_ex(ctx, params, n_params, prefix_c, cell_kind, input_size, hidden, embed, vocab, num_layers, num_bi_layers,
                           max_batch, max_src_len, beam, max_length, 0, out);
}

// GNMTEncoder.forward + the attention key projection; keeps mem / states inside the handle.
// mem_out (B,T,H) may be NULL.
static int gnmt_encode(tn_gnmt *g, const float *src, const float *table, int n_rows, int ld, const int32_t *row_idx,
                       const int32_t *valid_len, int batch, int steps, float *mem_out);
extern "C" int tn_gnmt_encode(tn_gnmt *g, const float *src, const int32_t *valid_len, int batch, int steps, float *mem_out) {
  TN_REQUIRE(g && src && valid_len, "tn_gnmt_encode: null argument");
  TN_REQUIRE(batch > 0 && batch <= g->maxB && steps > 0 && steps <= g->maxT, "tn_gnmt_encode: batch/steps exceed the handle");
  return gnmt_encode(g, src, nullptr, 0, 0, nullptr, valid_len, batch, steps, mem_out);
}
// tn_gnmt_encode from a device-resident feature table (tennis_hip.h): encoder layer 0's i2h product gathers its rows.
extern "C" int tn_gnmt_encode_rows(tn_gnmt *g, const float *table, int n_rows, int ld, const int32_t *row_idx, const int32_t *valid_len,
                                   int batch, int steps, float *mem_out) {
  TN_REQUIRE(g && table && row_idx && valid_len, "tn_gnmt_encode_rows: null argument");
  TN_REQUIRE(n_rows >= 1 && ld >= g->F, "tn_gnmt_encode_rows: needs n_rows >= 1 and ld >= the handle's input size");
  TN_REQUIRE(batch > 0 && batch <= g->maxB && steps > 0 && steps <= g->maxT, "tn_gnmt_encode_rows: batch/steps exceed the handle");
  return gnmt_encode(g, nullptr, table, n_rows, ld, row_idx, valid_len, batch, steps, mem_out);
}
static int gnmt_encode(tn_gnmt *g, const float *src, const float *table, int n_rows, int ld, const int32_t *row_idx,
                       const int32_t *valid_len, int batch, int steps, float *mem_out) {
  TN_ON_DEVICE(g->ctx->device);
  hipStream_t s = g->ctx->stream;
  const int H = g->H;
  TN_HIP_CHECK(hipMemcpyAsync(g->vl, valid_len, sizeof(int32_t) * batch, hipMemcpyDeviceToDevice, s));
  // layer i reads the previous layer's sequence and writes the other buffer; the last one writes mem.  Outputs past
  // valid_len are zero after every layer (tn_birnn_forward), so the closing SequenceMask (gnmt.py:159-161) is already applied.
  int rc = TN_OK;
  const float *in = src;
  for (int i = 0; i < g->NL; ++i) {
    float *outp = i == g->NL - 1 ? g->mem : (i & 1) ? g->seqB : g->seq0;
    if (i == 0 && row_idx) rc = birnn_forward_rows(g->enc[i], table, n_rows, ld, row_idx, batch, steps, g->vl, outp, g->hl[i], g->cl[i]);
    else rc = tn_birnn_forward(g->enc[i], in, batch, steps, g->vl, outp, g->hl[i], g->cl[i]);   // bi: hl / cl = [fwd, bwd] final states
    if (rc) return rc;
    if (g->residual && i > g->NBI)      // gnmt.py:155-157: outputs + inputs from the SECOND uni-directional layer on
      TN_TRY(launch_mul_add(outp, nullptr, in, outp, (long)batch * steps * H, s));
    in = outp;
  }
  TN_TRY(launch_linear_f32(g->mem, H, g->wk, H, nullptr, g->keyproj, H, batch * steps, H, H, 0, s));
  TN_TRY(launch_transpose_bth(g->keyproj, g->keyprojT, batch, steps, H, s));
  if (mem_out) TN_HIP_CHECK(hipMemcpyAsync(mem_out, g->mem, sizeof(float) * (size_t)batch * steps * H, hipMemcpyDeviceToDevice, s));
  g->B = batch; g->T = steps;
  return TN_OK;
}

// BeamSearchTranslator.translate after tn_gnmt_encode.  samples (B,beam,max_length+2) int32 padded
// with -1, scores (B,beam), valid_length (B,beam) are DEVICE buffers; *length_host receives the
// number of valid columns of `samples` (what the reference's sampler would have returned).
static int gnmt_beam_search(tn_gnmt *g, int bos, int eos, float alpha, float K, int max_length, int32_t *samples, float *scores,
                            int32_t *valid_length, int *length_host, float *attention);
extern "C" int tn_gnmt_beam_search(tn_gnmt *g, int bos, int eos, float alpha, float K, int max_length, int32_t *samples,
                                   float *scores, int32_t *valid_length, int *length_host) {
  TN_REQUIRE(g && samples && scores && valid_length && length_host, "tn_gnmt_beam_search: null argument");
  return gnmt_beam_search(g, bos, eos, alpha, K, max_length, samples, scores, valid_length, length_host, nullptr);
}
// tn_gnmt_beam_search that also returns the final hypotheses' attention weights (B, beam, maxL - 1, T), what the reference's
// decoder hands up as step_additional_outputs with output_attention=True (gnmt.py:302-303,402-403)
extern "C" int tn_gnmt_beam_search_attention(tn_gnmt *g, int bos, int eos, float alpha, float K, int max_length, int32_t *samples,
                                             float *scores, int32_t *valid_length, int *length_host, float *attention) {
  TN_REQUIRE(g && samples && scores && valid_length && length_host && attention, "tn_gnmt_beam_search_attention: null argument");
  return gnmt_beam_search(g, bos, eos, alpha, K, max_length, samples, scores, valid_length, length_host, attention);
}
static int gnmt_beam_search(tn_gnmt *g, int bos, int eos, float alpha, float K, int max_length, int32_t *samples, float *scores,
                            int32_t *valid_length, int *length_host, float *attention) {
  TN_REQUIRE(g->B > 0, "tn_gnmt_beam_search: call tn_gnmt_encode first");
  TN_REQUIRE(max_length >= 1 && max_length + 2 <= g->maxL, "tn_gnmt_beam_search: max_length exceeds the handle");
  TN_REQUIRE(bos >= 0 && bos < g->V && eos >= 0 && eos < g->V, "tn_gnmt_beam_search: bos/eos outside the vocabulary");
  TN_ON_DEVICE(g->ctx->device);
  hipStream_t s = g->ctx->stream;
  const int B = g->B, T = g->T, H = g->H, E = g->E, V = g->V, beam = g->beam, R = B * beam, L = g->maxL;
  const int K0 = E + 2 * H, K1 = 3 * H;
  const bool lstm = g->G == 4;
  TN_REQUIRE(beam_lds_bytes(H, V, beam, beam_split(H, V, beam, kStepLdsMax)) <= kStepLdsMax && att_split(T, H, kStepLdsMax) > 0,
             "tn_gnmt_beam_search: beam * (2*hidden + 2*vocab) or 3 * max(hidden, source length) floats exceed the step kernels' 152 KiB of LDS");
  if (attention && !(g->att_hist && g->att_rows)) {      // the first search that asks: history and row table at the handle's capacities
    const size_t Rmax = (size_t)g->maxB * beam, Smax = (size_t)(g->maxL - 2);
    if (!g->att_hist) g->att_hist = g->pool.alloc<float>(Smax * Rmax * g->maxT);
    if (!g->att_rows) g->att_rows = g->pool.alloc<int32_t>(Rmax * Smax);
    if (!g->att_hist || !g->att_rows) {
      g->pool.failed = false;
      tn_set_error("tn_gnmt_beam_search_attention: device allocation failed");
      return TN_ERR_NOMEM;
    }
  }
  float *const hist = attention ? g->att_hist : nullptr;      // step i's rows at hist + i * R * T
  const size_t hist_step = (size_t)R * T;
  TN_HIP_CHECK(hipMemsetAsync(g->samples[0], 0xff, sizeof(int32_t) * (size_t)R * L, s));
  // decoder layer i starts from encoder layer i's state, the BACKWARD direction's for a bidirectional layer (gnmt.py:146-150,224-252)
  const int NL = g->NL, nmid = NL - 2;
  auto hinit = [&](int i) { return (const float *)(g->hl[i] + (i < g->NBI ? (size_t)B * H : 0)); };
  auto cinit = [&](int i) { return (const float *)(g->cl[i] + (i < g->NBI ? (size_t)B * H : 0)); };
  const bool fused0 = NL == 2;
  float *sx1 = fused0 ? g->sx1p : g->sx1;            // the last cell's step input, pitch ld1
  const int ld1 = fused0 ? -(g->maxB * beam) : K1;      // two layers: k-group-major, the form the gate GEMM reads (xidx)
  // first step's inputs: x0 = [embed(bos), 0, h0 of the clip], x1[:, 2H:3H] = h1 of the clip, cell states (LSTM)
  TN_TRY(launch_dec_prep(g->emb, nullptr, 0, bos, nullptr, 0, hinit(0), H, hinit(NL - 1), H, lstm ? cinit(0) : nullptr, cinit(NL - 1), g->sx0, sx1,
                         ld1, g->c0cur, g->c1cur, beam, R, H, E, s));
  for (int j = 0; j < nmid; ++j)
    TN_TRY(launch_dec_mid_state(nullptr, hinit(j + 1), lstm ? cinit(j + 1) : nullptr, g->mid[j].sx, g->mid[j].ccur, true, beam, R, H, s));
  TN_TRY(launch_beam_init(g->scores, g->alive, g->vlen, g->tok, g->samples[0], L, B, beam, bos, s));
  // Two decoder layers (the reference's default): 3 launches per step.  The first cell's pre-activations g0 are linear in
  // x0 = [embed(word), ctx, h0]: step i + 1's attention kernel puts them together from ew[word] and the [h0, ctx] share p0 that
  // extra workgroups of step i's beam launch computed beside the clips (dec_beam_kernel).  More layers: the cells between
  // attention and the last one have their own operands, the first cell keeps its own GEMM (2 + 2 per layer launches).
  if (fused0 && !g->ew_ready) {      // embed . W0[:, 0:E]^T: (V, E) x (4H rows of K0, the first E columns) -> (V, 4H)
    TN_TRY(launch_linear_f32(g->emb, E, g->w0c, K0, nullptr, g->ew, 4 * H, V, 4 * H, E, 0, s));
    g->ew_ready = true;
  }
  float *h0buf[2] = {g->h0n, fused0 ? g->h0n2 : g->h0n}, *c0buf[2] = {g->c0n, fused0 ? g->c0n2 : g->c0n};
  DecAttentionArgs at;      // (what changes from step to step is filled in below)
  at.lstm = lstm; at.x1 = nmid ? g->mid[0].sx : sx1; at.ldx1 = nmid ? K1 : ld1;      // x1: input of the cell behind the attention
  at.kpT = g->keyprojT; at.mem = g->mem; at.valid_len = g->vl; at.ctx = g->ctxn; at.beam = beam; at.R = R; at.T = T; at.H = H; at.wpitch = T;
  DecBeamArgs bm;
  bm.g1 = g->g1; bm.x1 = sx1; bm.K1 = ld1; bm.lstm = lstm; bm.c1cur = g->c1cur; bm.wpT = g->wpT; bm.bp = g->bpp; bm.h0n = g->h0n; bm.ctx = g->ctxn;
  bm.c0n = g->c0n; bm.x0 = g->sx0; bm.c0cur = g->c0cur; bm.emb = g->emb; bm.B = B; bm.H = H; bm.E = E; bm.V = V; bm.beam = beam; bm.eos = eos;
  bm.scores = g->scores; bm.alive = g->alive; bm.vlen = g->vlen; bm.bp_par = g->bp_par; bm.bp_word = g->bp_word; bm.any_alive = g->flag;
  bm.hstate = g->hstate; bm.parent_out = g->parent;
  if (fused0) { bm.tok_out = g->tok; bm.w1x = g->w1x; bm.b1x = g->b1x; bm.K1p = g->K1p; bm.p0 = g->p0; }
  int steps_done = 0, all_dead = 0;
  // the loop is bound by launch-to-launch dependency latency, not by arithmetic
  for (int i = 0; i < max_length; ++i) {
    const int step = i + 1, cur = step & 1;
    if ((i & 15) == 0) TN_HIP_CHECK(hipMemsetAsync(g->flag, 0, sizeof(int32_t), s));
    at.hn = h0buf[cur]; at.cn = c0buf[cur]; at.wsave = hist ? hist + (size_t)i * hist_step : nullptr;
    if (!fused0 || i == 0) {
      TN_TRY(launch_linear_f32_lat(g->sx0, K0, g->w0c, K0, g->b0c, g->g0, 4 * H, R, 4 * H, K0, s));
      at.g0 = g->g0; at.hprev = g->sx0 + E + H; at.ldh = K0; at.cprev = g->c0cur;
    } else {      // g0 = ew[word] + p0[parent], the previous step's states by parent row
      at.g0 = nullptr; at.hprev = h0buf[cur ^ 1]; at.ldh = H; at.cprev = c0buf[cur ^ 1];
      at.tok = g->tok; at.par = g->parent; at.ew = g->ew; at.p0 = g->p0;
    }
    TN_TRY(launch_dec_attention(at, s));
    for (int j = 0; j < nmid; ++j) {
      GnmtMid &m = g->mid[j];
      float *xnext = j + 1 < nmid ? g->mid[j + 1].sx : g->sx1;
      TN_TRY(launch_linear_f32_lat(m.sx, K1, m.w, K1, m.b, m.g, 4 * H, R, 4 * H, K1, s));
      TN_TRY(launch_dec_cell(m.g, m.sx, lstm, m.ccur, m.hn, m.cn, nullptr, g->residual, xnext, K1, xnext + H, R, H, s));
    }
    TN_TRY(fused0 ? launch_linear_f32_lat_wk4(sx1, ld1, g->w1k4, g->b1c, g->g1, 4 * H, R, 4 * H, K1, s)
                  : launch_linear_f32_lat(g->sx1, K1, g->w1c, K1, g->b1c, g->g1, 4 * H, R, 4 * H, K1, s));
    // BeamSearchScorer [EXT gluonnlp]: length penalty ((K + length) / (K + 1)) ^ alpha of this step and of the previous one
    bm.step = step;
    bm.lp = powf(K + (float)step, alpha) / powf(K + 1.f, alpha);
    bm.prev_lp = step == 1 ? 1.f : powf(K + (float)(step - 1), alpha) / powf(K + 1.f, alpha);
    TN_TRY(launch_dec_beam(bm, s));
    for (int j = 0; j < nmid; ++j)      // the middle layers' states follow their rows' parent beams
      TN_TRY(launch_dec_mid_state(g->parent, g->mid[j].hn, lstm ? g->mid[j].cn : nullptr, g->mid[j].sx, g->mid[j].ccur, false, beam, R, H, s));
    steps_done = step;
    if ((i & 15) == 15 || i == max_length - 1) {   // look at the device flag every 16 steps
      int32_t f = 1;
      TN_HIP_CHECK(hipMemcpyAsync(&f, g->flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      TN_HIP_CHECK(hipStreamSynchronize(s));
      if (!f) { all_dead = 1; break; }
    }
  }
  // the token prefixes, from the back-pointers of the steps taken
  TN_TRY(launch_beam_samples(g->bp_par, g->bp_word, g->samples[0], L, steps_done, B, beam, bos, s));
  if (attention)      // the hypotheses' ancestor rows, then their weights out of the history
    TN_TRY(launch_beam_attention(g->bp_par, g->bp_word, hist, g->att_rows, attention, steps_done, B, beam, T, L - 1, s));
  if (!all_dead) {
    TN_TRY(launch_beam_finalize(g->alive, g->vlen, g->samples[0], L, steps_done + 1, R, eos, s));
    *length_host = steps_done + 2;
  }
  TN_HIP_CHECK(hipMemcpyAsync(samples, g->samples[0], sizeof(int32_t) * (size_t)R * L, hipMemcpyDeviceToDevice, s));
  TN_HIP_CHECK(hipMemcpyAsync(scores, g->scores, sizeof(float) * R, hipMemcpyDeviceToDevice, s));
  TN_HIP_CHECK(hipMemcpyAsync(valid_length, g->vlen, sizeof(int32_t) * R, hipMemcpyDeviceToDevice, s));
  if (all_dead) {   // the sampler returns as soon as every beam has finished: width = longest sample
    std::vector<int32_t> vl(R);
    TN_HIP_CHECK(hipMemcpyAsync(vl.data(), g->vlen, sizeof(int32_t) * R, hipMemcpyDeviceToHost, s));
    TN_HIP_CHECK(hipStreamSynchronize(s));
    int mx = 0;
    for (int v : vl) mx = v > mx ? v : mx;
    *length_host = mx;
  }
  return TN_OK;
}

// Teacher-forced decoding, NMTModel.forward -> GNMTDecoder.decode_seq (reference
// models/captioning/gnmt.py:254-304) as called by evaluate() (train_gnmt.py:280): feeds
// tgt[:, 0..L-1] one step at a time from the encoder state left by tn_gnmt_encode and writes the
// projected logits (B, L, V).  tgt is a DEVICE (B, ld) int32 array.
static int gnmt_decode_seq(tn_gnmt *g, const int32_t *tgt, int ld, int steps, float *logits, float *attention);
extern "C" int tn_gnmt_decode_seq(tn_gnmt *g, const int32_t *tgt, int ld, int steps, float *logits) {
  TN_REQUIRE(g && tgt && logits, "tn_gnmt_decode_seq: null argument");
  return gnmt_decode_seq(g, tgt, ld, steps, logits, nullptr);
}
// tn_gnmt_decode_seq that also returns every step's attention weights (B, steps, T): decode_seq with output_attention=True
// stacks the attention cell's weights as additional outputs (gnmt.py:302-303,402-403).  The step kernel stores row b of step i
// straight at attention[b, i, :] (row pitch steps * T).
extern "C" int tn_gnmt_decode_seq_attention(tn_gnmt *g, const int32_t *tgt, int ld, int steps, float *logits, float *attention) {
  TN_REQUIRE(g && tgt && logits && attention, "tn_gnmt_decode_seq_attention: null argument");
  return gnmt_decode_seq(g, tgt, ld, steps, logits, attention);
}
static int gnmt_decode_seq(tn_gnmt *g, const int32_t *tgt, int ld, int steps, float *logits, float *attention) {
  TN_REQUIRE(g->B > 0, attention ? "tn_gnmt_decode_seq_attention: call tn_gnmt_encode first" : "tn_gnmt_decode_seq: call tn_gnmt_encode first");
  TN_REQUIRE(steps >= 1 && ld >= steps, "tn_gnmt_decode_seq: bad target length");
  TN_ON_DEVICE(g->ctx->device);
  hipStream_t s = g->ctx->stream;
  const int B = g->B, T = g->T, H = g->H, E = g->E, V = g->V, R = B, K0 = E + 2 * H, K1 = 3 * H;
  const bool lstm = g->G == 4;
  TN_REQUIRE(att_split(T, H, kStepLdsMax) > 0, "tn_gnmt_decode_seq: 3 * max(hidden, source length) floats exceed the step kernel's 152 KiB of LDS");
  const int NL = g->NL, nmid = NL - 2;
  auto hinit = [&](int i) { return (const float *)(g->hl[i] + (i < g->NBI ? (size_t)B * H : 0)); };
  auto cinit = [&](int i) { return (const float *)(g->cl[i] + (i < g->NBI ? (size_t)B * H : 0)); };
  float *proj_in = g->residual ? g->hstate : g->h1n;     // use_residual: the projection sees h + the last cell's input
  DecAttentionArgs at;
  at.g0 = g->g0; at.hprev = g->sx0 + E + H; at.ldh = K0; at.cprev = g->c0cur; at.lstm = lstm; at.hn = g->h0n; at.cn = g->c0n;
  at.x1 = nmid ? g->mid[0].sx : g->sx1; at.ldx1 = K1; at.kpT = g->keyprojT; at.mem = g->mem; at.valid_len = g->vl; at.ctx = g->ctxn;
  at.R = R; at.T = T; at.H = H; at.wpitch = (long)steps * T;
  for (int i = 0; i < steps; ++i) {
    // decoder layer j starts from encoder layer j's state, the BACKWARD direction's for a bidirectional layer (gnmt.py:146-150,224-252)
    const float *h0p = i ? g->h0n : hinit(0), *h1p = i ? g->h1n : hinit(NL - 1);
    const float *c0p = !lstm ? nullptr : i ? g->c0n : cinit(0), *c1p = !lstm ? nullptr : i ? g->c1n : cinit(NL - 1);
    TN_TRY(launch_dec_prep(g->emb, tgt, ld, i, i ? g->ctxn : nullptr, H, h0p, H, h1p, H, c0p, c1p, g->sx0, g->sx1, K1, g->c0cur, g->c1cur, 1, R, H,
                           E, s));
    for (int j = 0; j < nmid; ++j)
      TN_TRY(launch_dec_mid_state(nullptr, i ? g->mid[j].hn : hinit(j + 1), !lstm ? nullptr : i ? g->mid[j].cn : cinit(j + 1), g->mid[j].sx,
                                  g->mid[j].ccur, false, 1, R, H, s));
    TN_TRY(launch_linear_f32_lat(g->sx0, K0, g->w0c, K0, g->b0c, g->g0, 4 * H, R, 4 * H, K0, s));
    at.wsave = attention ? attention + (size_t)i * T : nullptr;
    TN_TRY(launch_dec_attention(at, s));
    for (int j = 0; j < nmid; ++j) {
      GnmtMid &m = g->mid[j];
      float *xnext = j + 1 < nmid ? g->mid[j + 1].sx : g->sx1;
      TN_TRY(launch_linear_f32_lat(m.sx, K1, m.w, K1, m.b, m.g, 4 * H, R, 4 * H, K1, s));
      TN_TRY(launch_dec_cell(m.g, m.sx, lstm, m.ccur, m.hn, m.cn, nullptr, g->residual, xnext, K1, xnext + H, R, H, s));
    }
    TN_TRY(g->w1k4 ? launch_linear_f32_lat_wk4(g->sx1, K1, g->w1k4, g->b1c, g->g1, 4 * H, R, 4 * H, K1, s)      // (two layers: the k-group-major copy)
                   : launch_linear_f32_lat(g->sx1, K1, g->w1c, K1, g->b1c, g->g1, 4 * H, R, 4 * H, K1, s));
    TN_TRY(launch_dec_cell(g->g1, g->sx1, lstm, g->c1cur, g->h1n, g->c1n, nullptr, g->residual, g->residual ? g->hstate : nullptr, H, nullptr, R, H, s));
    TN_TRY(launch_linear_f32_lat(proj_in, H, g->wp, H, g->bp, logits + (size_t)i * V, steps * V, R, V, H, s));
  }
  return TN_OK;
}

// MaskedSoftmaxCELoss of gluonnlp as used at reference train_gnmt.py:256,281: loss (B,) =
// mean over the L steps of the label's negative log-probability, masked by valid_len.
extern "C" int tn_masked_softmax_ce(tn_ctx *ctx, const float *logits, const int32_t *labels, int ld_labels,
                                    const int32_t *valid_len, int batch, int steps, int vocab, float *loss) {
  TN_REQUIRE(ctx && logits && labels && valid_len && loss, "tn_masked_softmax_ce: null argument");
  TN_REQUIRE(batch > 0 && steps > 0 && vocab > 0 && ld_labels >= steps, "tn_masked_softmax_ce: bad shape");
  TN_ON_DEVICE(ctx->device);
  return launch_masked_ce(logits, labels, ld_labels, valid_len, loss, batch, steps, vocab, ctx->stream);
}

extern "C" int tn_gnmt_destroy(tn_gnmt *g) {
  if (!g) return TN_OK;
  TnDeviceGuard tn_dg_(g->ctx->device);
  for (tn_birnn *e : g->enc) tn_birnn_destroy(e);
  g->pool.release();
  delete g;
  return TN_OK;
}
