// The parameters of a training handle, written once: ParamMap finds what the caller passed by name, ParamTable says where each
// name lives inside the handle (create loads through it, *_read_param reads through it, tn_dbg_trainer_params lists it), and the
// three builders below are the one place that knows the order of the flat buffers.  Host only: no HIP call, no device.
#pragma once
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/tennis_hip.h"

void tn_set_error(const std::string &msg);

struct ParamMap {
  std::map<std::string, const tn_param *> m;
  ParamMap(const tn_param *p, int n) {
    for (int i = 0; i < n; ++i) m[p[i].name] = &p[i];
  }
  int64_t numel(const std::string &name) const {      // -1: not there
    auto it = m.find(name);
    return it == m.end() ? -1 : it->second->numel;
  }
  const float *get(const std::string &name, int64_t numel) const {
    auto it = m.find(name);
    if (it == m.end()) {
      tn_set_error("missing parameter: " + name);
      return nullptr;
    }
    if (it->second->numel != numel) {
      tn_set_error("parameter " + name + " has the wrong size: " + std::to_string(it->second->numel) + " elements, expected " +
                   std::to_string(numel));
      return nullptr;
    }
    return it->second->data_host;
  }
};

// conv weight (O, I, kh, kw) as Gluon stores it <-> the GEMM layout (O, kh*kw*I) the fine-tuning step keeps
inline void conv_to_gemm(const float *src, float *dst, int O, int I, int kh, int kw) {
  for (int o = 0; o < O; ++o)
    for (int i = 0; i < I; ++i)
      for (int y = 0; y < kh; ++y)
        for (int x = 0; x < kw; ++x) dst[((long)o * kh * kw + y * kw + x) * I + i] = src[(((long)o * I + i) * kh + y) * kw + x];
}
inline void conv_from_gemm(const float *src, float *dst, int O, int I, int kh, int kw) {
  for (int o = 0; o < O; ++o)
    for (int i = 0; i < I; ++i)
      for (int y = 0; y < kh; ++y)
        for (int x = 0; x < kw; ++x) dst[(((long)o * I + i) * kh + y) * kw + x] = src[((long)o * kh * kw + y * kw + x) * I + i];
}

struct ParamTable {
  enum Where { FLAT = 0, STATE = 1, PTR = 2 };   // the flat parameter / gradient buffers, the state buffer, a device pointer of its own
  struct Row {
    std::string name;
    Where where;
    long off, count;             // off: floats into the flat buffers or the state buffer; PTR: 0
    const float *ptr = nullptr;  // PTR rows: set by create once the buffer exists
    int O = 0, I = 0, kh = 0, kw = 0;   // O > 0: a convolution weight kept in the GEMM layout
  };
  std::vector<Row> rows;
  std::map<std::string, int> index;
  long n = 0, ns = 0;            // floats of the flat buffers / of the state buffer

  long add(const std::string &name, long count, Where where = FLAT) {      // -> the offset
    long &end = where == STATE ? ns : n;
    const long off = where == PTR ? 0 : end;
    if (where != PTR) end += count;
    index[name] = (int)rows.size();
    rows.push_back(Row{name, where, off, count});
    return off;
  }
  long add_conv(const std::string &name, int O, int I, int kh, int kw) {
    const long off = add(name, (long)O * I * kh * kw);
    Row &r = rows.back();
    r.O = O; r.I = I; r.kh = kh; r.kw = kw;
    return off;
  }
  const Row *find(const std::string &name) const {
    auto it = index.find(name);
    return it == index.end() ? nullptr : &rows[it->second];
  }
  void set_ptr(const std::string &name, const float *p) { rows[index.at(name)].ptr = p; }
  // every FLAT row into w (n floats), every STATE row into st (ns floats); false with the error set at the first name that is
  // missing or has another size
  bool load(const ParamMap &pm, std::vector<float> &w, std::vector<float> &st) const {
    w.assign(n, 0.f); st.assign(ns, 0.f);
    for (const Row &r : rows) {
      if (r.where == PTR) continue;
      const float *src = pm.get(r.name, r.count);
      if (!src) return false;
      float *dst = (r.where == STATE ? st.data() : w.data()) + r.off;
      if (r.O) conv_to_gemm(src, dst, r.O, r.I, r.kh, r.kw);
      else memcpy(dst, src, sizeof(float) * r.count);
    }
    return true;
  }
};

// ---- temporal head: wi[l,r], bi[l,r], wh[l,r], bh[l,r], wd, bd ------------------------------------------------------------
struct HeadOffsets { long o_wi, o_bi, o_wh, o_bh, o_wd, o_bd; };
inline ParamTable head_param_table(int G, int F, int H, int C, const std::string &rnn_prefix, const std::string &dense_prefix,
                                   HeadOffsets *o) {
  ParamTable t;
  const long GH = (long)G * H;
  const std::string l = rnn_prefix + "l0_", r = rnn_prefix + "r0_";
  o->o_wi = t.add(l + "i2h_weight", GH * F); t.add(r + "i2h_weight", GH * F);
  o->o_bi = t.add(l + "i2h_bias", GH); t.add(r + "i2h_bias", GH);
  o->o_wh = t.add(l + "h2h_weight", GH * H); t.add(r + "h2h_weight", GH * H);
  o->o_bh = t.add(l + "h2h_bias", GH); t.add(r + "h2h_bias", GH);
  o->o_wd = t.add(dense_prefix + "weight", (long)C * 2 * H);
  o->o_bd = t.add(dense_prefix + "bias", C);
  return t;
}

// ---- captioner: per encoder layer wi, bi, wh, bh (the directions adjacent inside each), per decoder cell the same, then
// wk, wp, bp, emb ---------------------------------------------------------------------------------------------------------
struct CellOffsets { long o_wi, o_bi, o_wh, o_bh; };
struct GnmtOffsets { std::vector<CellOffsets> enc, dec; long o_wk, o_wp, o_bp, o_emb; };
inline int gnmt_enc_dirs(int i, int NBI) { return i < NBI ? 2 : 1; }
inline int gnmt_enc_in(int i, int F, int H, int NBI) { return i == 0 ? F : gnmt_enc_dirs(i - 1, NBI) * H; }
inline int gnmt_dec_in(int j, int H, int E) { return j == 0 ? E + H : 2 * H; }
inline ParamTable gnmt_param_table(int G, int F, int H, int E, int V, int NL, int NBI, const std::string &pre, GnmtOffsets *o) {
  ParamTable t;
  const long GH = (long)G * H;
  // one tensor kind of a cell, once per direction: -> the offset of the first
  auto kind = [&](const std::string &cell, int D, const char *what, long count) {
    long first = -1;
    for (int d = 0; d < D; ++d) {
      const long off = t.add(pre + cell + (D == 2 ? (d ? "_r_" : "_l_") : "_") + what, count);
      if (d == 0) first = off;
    }
    return first;
  };
  auto cell = [&](const std::string &name, int D, long in) {
    CellOffsets c;
    c.o_wi = kind(name, D, "i2h_weight", GH * in); c.o_bi = kind(name, D, "i2h_bias", GH);
    c.o_wh = kind(name, D, "h2h_weight", GH * H); c.o_bh = kind(name, D, "h2h_bias", GH);
    return c;
  };
  o->enc.clear(); o->dec.clear();
  for (int i = 0; i < NL; ++i) o->enc.push_back(cell("enc_rnn" + std::to_string(i), gnmt_enc_dirs(i, NBI), gnmt_enc_in(i, F, H, NBI)));
  for (int j = 0; j < NL; ++j) o->dec.push_back(cell("dec_rnn" + std::to_string(j), 1, gnmt_dec_in(j, H, E)));
  o->o_wk = t.add(pre + "dec_attention_key_weight", (long)H * H);
  o->o_wp = t.add(pre + "tgt_proj_weight", (long)V * H);
  o->o_bp = t.add(pre + "tgt_proj_bias", V);
  o->o_emb = t.add(pre + "tgt_embed_weight", (long)V * E);
  return t;
}

// ---- DenseNet-121 backbone: conv0, bn0; per block, per layer bn1, w1, bn2, w3; after blocks 1-3 the transition's bn, w; the
// final bn; dense w, b with a classifier.  gamma / beta in the flat buffers, the running statistics in the same walk in the state
// buffer, the batch statistics of the last step ("<bn>_batch_mean" / "_batch_var", test hook) behind pointers of their own. ---
struct FtBn {
  long o_gamma, o_beta, o_rm, o_rv;
  int C;
  std::string name;
  float *mean = nullptr, *var = nullptr;   // batch statistics
  // the folded form relu(x * sc + sh) of the layer's training-mode BatchNorm + ReLU, refreshed in every forward - what the GEMMs'
  // operand transforms and the fused im2col read instead of a stored activation
  float *sc = nullptr, *sh = nullptr;
};
struct FtLayer { FtBn bn1, bn2; long o_w1, o_w3; int K; float *z1 = nullptr; };
struct FtTrans { FtBn bn; long o_w; int Cin, Cout; float *z = nullptr; };
struct FtNet {
  long o_w0, o_wd = -1, o_bd = -1;
  FtBn bn0, bnF;
  std::vector<FtLayer> layers[4];
  FtTrans trans[3];
  int Cin[4], Ctot[4];
  template <typename Fn>
  void each_bn(Fn fn) {
    fn(bn0); fn(bnF);
    for (int b = 0; b < 4; ++b) {
      for (FtLayer &L : layers[b]) { fn(L.bn1); fn(L.bn2); }
      if (b < 3) fn(trans[b].bn);
    }
  }
};
// cls null: the backbone alone, no classifier
inline ParamTable ft_param_table(const std::string &pre, const char *cls, int classes, FtNet *f) {
  ParamTable t;
  static const int kCfg[4] = {6, 12, 24, 16};
  auto mkbn = [&](const std::string &name, int C) {
    FtBn b;
    b.name = name; b.C = C;
    b.o_gamma = t.add(name + "_gamma", C); b.o_beta = t.add(name + "_beta", C);
    b.o_rm = t.add(name + "_running_mean", C, ParamTable::STATE); b.o_rv = t.add(name + "_running_var", C, ParamTable::STATE);
    t.add(name + "_batch_mean", C, ParamTable::PTR); t.add(name + "_batch_var", C, ParamTable::PTR);
    return b;
  };
  f->o_w0 = t.add_conv(pre + "conv0_weight", 64, 3, 7, 7);
  f->bn0 = mkbn(pre + "batchnorm0", 64);
  int c = 64, outer = 1;
  for (int b = 0; b < 4; ++b) {
    const std::string sp = pre + "stage" + std::to_string(b + 1) + "_";
    f->Cin[b] = c;
    f->layers[b].clear();
    for (int l = 0; l < kCfg[b]; ++l) {
      FtLayer L;
      L.K = c + 32 * l;
      L.bn1 = mkbn(sp + "batchnorm" + std::to_string(2 * l), L.K);
      L.o_w1 = t.add(sp + "conv" + std::to_string(2 * l) + "_weight", 128L * L.K);
      L.bn2 = mkbn(sp + "batchnorm" + std::to_string(2 * l + 1), 128);
      L.o_w3 = t.add_conv(sp + "conv" + std::to_string(2 * l + 1) + "_weight", 32, 128, 3, 3);
      f->layers[b].push_back(L);
    }
    c += 32 * kCfg[b];
    f->Ctot[b] = c;
    if (b < 3) {
      FtTrans &T = f->trans[b];
      T.Cin = c; T.Cout = c / 2;
      T.bn = mkbn(pre + "batchnorm" + std::to_string(outer), c);
      T.o_w = t.add(pre + "conv" + std::to_string(outer) + "_weight", (long)T.Cout * T.Cin);
      c /= 2;
      ++outer;
    }
  }
  f->bnF = mkbn(pre + "batchnorm" + std::to_string(outer), c);
  if (cls) {
    f->o_wd = t.add(std::string(cls) + "weight", (long)classes * c);
    f->o_bd = t.add(std::string(cls) + "bias", classes);
  }
  return t;
}
