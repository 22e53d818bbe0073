// The DenseNet-121 frame encoder of libtennis_hip.so (include/tennis_hip.h): weight folding / packing at create, the launch
// schedule of a forward pass (the routes of the dense blocks: encoder_plan.h), the fp32 and fp32x3 modes, calibration and taps.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "api_internal.h"
#include "encoder_plan.h"

namespace {

constexpr float kBnEps = 1e-5f;

// Folded inference BatchNorm: y = x*scale + shift.
bool fold_bn(const ParamMap &pm, const std::string &name, int c, std::vector<float> &scale, std::vector<float> &shift) {
  const float *g = pm.get(name + "_gamma", c), *b = pm.get(name + "_beta", c);
  const float *mu = pm.get(name + "_running_mean", c), *var = pm.get(name + "_running_var", c);
  if (!g || !b || !mu || !var) return false;
  scale.resize(c);
  shift.resize(c);
  bn_scale_shift(g, b, mu, var, c, kBnEps, scale.data(), shift.data());
  return true;
}

// fp16 copy with 64 trailing zeros: the LDS-DMA k-tile of the fused dense layer may read up
// to 32 halfs past the last row when K % 64 == 32
std::vector<f16> to_f16(const float *w, size_t n) {
  std::vector<f16> h(n + 64, (f16)0.f);
  for (size_t i = 0; i < n; ++i) h[i] = (f16)w[i];
  return h;
}

// Exact-weights mode: w = hi + lo with hi = fp16(w), lo = fp16(w - hi) (22 bits of the fp32 weight survive).
// rows x k fp32 -> [rows][2 kp] fp16 = [hi (k, zero-padded to kp) | lo (...)], + 64 halves of slack like to_f16
std::vector<f16> split_hi_lo_rows(const float *w, int rows, int k, int kp) {
  std::vector<f16> h((size_t)rows * 2 * kp + 64, (f16)0.f);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < k; ++c) {
      const float v = w[(size_t)r * k + c];
      const f16 hi = (f16)v;
      h[(size_t)r * 2 * kp + c] = hi;
      h[(size_t)r * 2 * kp + kp + c] = (f16)(v - (float)hi);
    }
  return h;
}

}  // namespace
// 3x3 weights (32,128,3,3) -> MFMA B fragments [72 k-steps][64 lanes][8]:
// k-step s = tap*8 + kk; lane l: n = l&31, channel = kk*16 + (l>>5)*8 + j.
std::vector<f16> pack_conv3x3(const float *w) {
  // two MFMA operand layouts back to back (72*64*8 halves each):
  //  [0]     v_mfma_f32_32x32x16_f16 A fragments [9 taps x 8 k16-steps][64 lanes][8]   (conv3x3.hip)
  //  [36864] v_mfma_f32_16x16x32_f16 A fragments [9 taps][4 k32-steps][2 n-frags][64 lanes][8]   (dense_layer_big.hip):
  //          lane l: out channel nf*16 + (l&15), in channel kk*32 + (l>>4)*8 + j
  std::vector<f16> p((size_t)2 * 72 * 64 * 8);
  for (int s = 0; s < 72; ++s) {
    const int tap = s >> 3, kk = s & 7, ky = tap / 3, kx = tap % 3;
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 8; ++j) {
        const int n = l & 31, c = kk * 16 + (l >> 5) * 8 + j;
        p[((size_t)s * 64 + l) * 8 + j] = (f16)w[(((size_t)n * 128 + c) * 3 + ky) * 3 + kx];
      }
  }
  f16 *q = p.data() + (size_t)72 * 64 * 8;
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap % 3;
    for (int kk = 0; kk < 4; ++kk)
      for (int nf = 0; nf < 2; ++nf)
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 8; ++j) {
            const int n = nf * 16 + (l & 15), c = kk * 32 + (l >> 4) * 8 + j;
            q[((((size_t)tap * 4 + kk) * 2 + nf) * 64 + l) * 8 + j] = (f16)w[(((size_t)n * 128 + c) * 3 + ky) * 3 + kx];
          }
  }
  return p;
}
namespace {

// stem weights (64,3,7,7) -> MFMA A fragments [7 ky][4 nfrag][64 lanes][8]:
// lane l: n = nf*16 + (l&15); k slot (l>>4)*8 + j -> x-tap kx = slot>>2, channel c = slot&3 (the eighth tap is zero);
// zero_first: the zero tap comes first, kx = (slot>>2) - 1 (operand alignment of the fused stem + maxpool kernel).
std::vector<f16> pack_stem(const float *w, bool zero_first) {
  std::vector<f16> p((size_t)7 * 4 * 64 * 8);
  for (int ky = 0; ky < 7; ++ky)
    for (int nf = 0; nf < 4; ++nf)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) {
          const int n = nf * 16 + (l & 15), slot = (l >> 4) * 8 + j, kx = (slot >> 2) - (zero_first ? 1 : 0), c = slot & 3;
          float v = 0.f;
          if (kx >= 0 && kx < 7 && c < 3) v = w[(((size_t)n * 3 + c) * 7 + ky) * 7 + kx];
          p[(((size_t)ky * 4 + nf) * 64 + l) * 8 + j] = (f16)v;
        }
  return p;
}

}  // namespace

// The stem's constants from conv0's weights (64,3,7,7) and batchnorm0's folded scale / shift: what tn_densenet121_create uploads and
// what the tn_dbg_stem hook runs the kernels on.  centre: m_c of the centred output (StemArgs::floor; nullptr: not centred, no floor).
StemFold fold_stem(const float *w0, const float *bn_scale, const float *bn_shift, const float *centre, bool exact) {
  StemFold f;
  std::vector<float> s(bn_scale, bn_scale + 64), t(bn_shift, bn_shift + 64);
  // the input normalisation's 1 / (255 std_c) goes into the weights before they are rounded (common.h "the stem's operand")
  std::vector<float> w0s((size_t)64 * 3 * 49), tu(64);
  for (int n = 0; n < 64; ++n) {
    double bias = 0.0;
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < 49; ++k) {
        const size_t i = ((size_t)n * 3 + c) * 49 + k;
        w0s[i] = w0[i] * stem_wfactor(c);
        bias -= (double)(float)(f16)w0s[i] * stem_pad(c);
      }
    s[n] = (float)((double)s[n] / kStemWScale);
    tu[n] = (float)((double)t[n] + (double)s[n] * bias);
  }
  f.wp = pack_stem(w0s.data(), false);
  f.wp_zf = pack_stem(w0s.data(), true);
  if (exact) {     // w = hi + lo: the second fragment image (the constant of the integer staging then uses hi + lo as well)
    std::vector<float> lo(w0s.size());
    for (int n = 0; n < 64; ++n) {
      double bias = 0.0;
      for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 49; ++k) {
          const size_t i = ((size_t)n * 3 + c) * 49 + k;
          const float hi = (float)(f16)w0s[i];
          lo[i] = w0s[i] - hi;
          bias -= ((double)hi + (double)(float)(f16)lo[i]) * stem_pad(c);
        }
      tu[n] = (float)((double)t[n] + (double)s[n] * bias);
    }
    f.wp_zf_lo = pack_stem(lo.data(), true);
  }
  if (centre) {
    f.floor.resize(64);
    for (int n = 0; n < 64; ++n) {
      t[n] = (float)((double)t[n] - (double)centre[n]);
      tu[n] = (float)((double)tu[n] - (double)centre[n]);
      f.floor[n] = -centre[n];
    }
  }
  f.scale = s; f.shift = t; f.shift_u8 = tu;
  return f;
}

// the same from batchnorm0's raw parameters (the tn_dbg_stem hook): folded as fold_bn folds them
StemFold fold_stem_bn(const float *w0, const float *gamma, const float *beta, const float *mean, const float *var, const float *centre, bool exact) {
  float s[64], t[64];
  bn_scale_shift(gamma, beta, mean, var, 64, kBnEps, s, t);
  return fold_stem(w0, s, t, centre, exact);
}

namespace {

struct EventTimer {  // brackets launches with HIP events when enabled
  bool on = false;
  hipStream_t s = nullptr;
  struct Rec { hipEvent_t a, b; int fam; };
  std::vector<Rec> recs;
  std::vector<tn_kernel_stat> fams;
  int family(const char *name) {
    for (size_t i = 0; i < fams.size(); ++i)
      if (!strcmp(fams[i].name, name)) return (int)i;
    tn_kernel_stat st;
    memset(&st, 0, sizeof(st));
    strncpy(st.name, name, sizeof(st.name) - 1);
    fams.push_back(st);
    return (int)fams.size() - 1;
  }
  void begin(const char *name, double flops, double bytes) {
    if (!on) return;
    Rec r;
    r.fam = family(name);
    (void)hipEventCreate(&r.a);
    (void)hipEventCreate(&r.b);
    fams[r.fam].launches += 1;
    fams[r.fam].flops += flops;
    fams[r.fam].bytes += bytes;
    (void)hipEventRecord(r.a, s);
    recs.push_back(r);
  }
  void end() {
    if (!on) return;
    (void)hipEventRecord(recs.back().b, s);
  }
  void finish() {
    if (!on) return;
    (void)hipStreamSynchronize(s);
    for (auto &r : recs) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, r.a, r.b);
      fams[r.fam].ms += ms;
      (void)hipEventDestroy(r.a);
      (void)hipEventDestroy(r.b);
    }
    recs.clear();
  }
};

}  // namespace

// ---- DenseNet-121 encoder --------------------------------------------------------
struct tn_encoder {
  tn_ctx *ctx;
  DevPool pool;
  int maxB;
  EncGeom geom;            // the maps of the input size (both fp32 modes use it too)
  EncPolicy policy;        // the switches the routing plan reads (encoder_plan.h)
  f16 *stem_wp, *stem_wp_zf, *stem_wp_zf_lo = nullptr;
  float *stem_scale, *stem_shift, *stem_shift_u8;
  float *stem_floor = nullptr;                               // centred stem output (round 6): the ReLU's floor -m_c on the device
  std::vector<float> stem_centre;                            // m_c on the host (read_tap / input_means add it back)
  std::vector<float> calib_centre;                           // per block-1 dense layer, 64 each: m_c, or 0 where the layer's clamp is a constant (lo == hi)
  struct DenseLayer { float *s1, *t1; f16 *w1; float *s2, *t2; f16 *w3p; int cin; f16 *w1s = nullptr, *w3s = nullptr; };   // w1s / w3s: fragment images of the strip kernel
  std::vector<DenseLayer> layers[4];
  struct Trans { float *s, *t; f16 *w; int cin, cout; f16 *wfrag = nullptr; } trans[3];      // wfrag: w in MFMA operand order (trans_ws.hip)
  float *head_s, *head_t;
  float *zeros128 = nullptr;   // a BatchNorm shift of zeros (un-fused dense layers: the shift was added by the 1x1)
  f16 *stem_out, *bott, *blockbuf[4];
  // the last block's map once more in fp32, written by the last transition and the 7x7 block kernel: what the head and the class
  // activation maps read where those two kernels do not apply the head themselves (encoder_plan.h::enc_head_fused - then nothing
  // writes or reads it: the instrumented pass, tn_densenet121_forward_class_maps and TN_NO_HEAD_FUSE are its users)
  float *head32 = nullptr;
  // tn_densenet121_forward_class_maps: set for the duration of that call only.  Every range of the call launches class_maps_kernel
  // behind its head, on the map that head read, and writes the maps of its frames at their offset in cam_out.
  const float *cam_w = nullptr;   // the Dense weight (cam_units, feat_dim), nullptr: no maps (every other entry point)
  float *cam_out = nullptr;       // (batch, cam_units, 7 PH, 7 PW)
  int cam_units = 0;
  size_t workspace_bytes;
  int last_batch;
  bool split;
  int nsplit;                 // side streams in use (TN_SPLIT, default 2)
  DenseLayerDev *chain_dev[4] = {nullptr, nullptr, nullptr, nullptr};
  DenseStripLayerDev *strip_chain_dev[4] = {nullptr, nullptr, nullptr, nullptr};   // argument table of the chained strip launch (enc_strip_chain_layers)
  float *calib_dev = nullptr;   // tn_densenet121_input_means: where the layer-wise pass leaves the mean of every convolution's input
  double *calib_scratch = nullptr;
  float *ones128 = nullptr;
  DenseBlock7Args b7[4] = {};  // packed operands of the LDS-resident 7x7 kernel per block (enc_block7; wa == nullptr: not packed)
  DenseStreamArgs b_stream[4] = {};                             // packed operands of the streamed kernel per block (enc_stream_kernel; stream == nullptr: not packed)
  f16 *b_stream_scratch[4] = {nullptr, nullptr, nullptr, nullptr};   // the kernel's k-step-major working copy of the block's frames
  hipStream_t side[4];
  hipEvent_t ev_in, ev_done[2][4];   // completion of the side streams, alternating per forward call
  bool pipelined = false;            // tn_densenet121_set_pipelined: the caller's stream is not made to wait inside forward
  bool last_interleaved = false;     // the previous split call took the whole-batch form
  int last_ws0 = 0;                  // first workspace frame slot of the last forward (read_tap)
  bool interleave = false;           // pipelined calls run WHOLE batches on alternating side streams (round 6, encoder_run), on two workspace sets
  long calls = 0;                    // forward calls so far
  int split_of[2] = {0, 0};          // side streams the call of each parity used (0: it ran on the caller's stream)
  int split_batch = 0;               // batch size of the last split call (pipelined calls share the workspace by row range)
  // TN_ENC_FP32 (dense_fp32.hip): fp32 weights, fp32 activations, f32-input MFMA.  Nothing above this is packed or allocated
  // for such an encoder, and nothing below for any other.
  bool fp32 = false;
  // TN_ENC_FP32X3 (dense_fp32x3.hip): an fp32-mode encoder (fp32 is set as well) whose convolutions run on the bf16 MFMA from
  // three-term weight images (the *x members: fp32x3_pack_weights of the fp32 arrays beside them, nullptr in the fp32 mode)
  bool fp32x3 = false;
  struct Fp32Layer { float *s1, *t1, *w1, *s2, *t2, *w3; int cin; uint16_t *w1x, *w3x; };   // w1 [cin][128], w3 [9 * 128][32] (k = tap * 128 + c)
  struct Fp32Net {
    float *stem_w = nullptr, *stem_s = nullptr, *stem_t = nullptr;      // stem_w [160][64] (k = c * 49 + ky * 7 + kx, zero past 147)
    uint16_t *stem_wx = nullptr;
    std::vector<Fp32Layer> layers[4];
    struct { float *s, *t, *w; int cin, cout; uint16_t *wx; } trans[3];   // w [cin][cout]
    float *head_s = nullptr, *head_t = nullptr;
    float *stem = nullptr, *bott = nullptr, *buf[4] = {nullptr, nullptr, nullptr, nullptr};   // workspace: stem map, bottleneck, concat buffers
  } f32;
};

// ---- TN_ENC_FP32: the raw fp32 parameters, BatchNorms folded in double and rounded to fp32 once ----
static bool fold_bn_f64(const ParamMap &pm, const std::string &name, int c, std::vector<float> &scale, std::vector<float> &shift) {
  const float *g = pm.get(name + "_gamma", c), *b = pm.get(name + "_beta", c);
  const float *mu = pm.get(name + "_running_mean", c), *var = pm.get(name + "_running_var", c);
  if (!g || !b || !mu || !var) return false;
  scale.resize(c);
  shift.resize(c);
  for (int i = 0; i < c; ++i) {
    const double s = (double)g[i] / std::sqrt((double)var[i] + 1e-5);
    scale[i] = (float)s;
    shift[i] = (float)((double)b[i] - (double)mu[i] * s);
  }
  return true;
}

// w (rows, k) row-major -> [kp][rows] (k-major, the GEMM's B operand), zero rows past k
static std::vector<float> transpose_pad(const float *w, int rows, int k, int kp) {
  std::vector<float> o((size_t)kp * rows, 0.f);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < k; ++c) o[(size_t)c * rows + r] = w[(size_t)r * k + c];
  return o;
}

static int create_fp32(tn_encoder *e, const ParamMap &pm, const std::string &pre) {
  auto &F = e->f32;
  std::vector<float> s, t;
  // the B operand [kp][n] of a convolution: the fp32 array and - fp32x3 - its three-term bf16 image
  auto upload_w = [&](const std::vector<float> &wk, int kp, int n, uint16_t *&wx) {
    wx = e->fp32x3 ? e->pool.upload(fp32x3_pack_weights(wk.data(), kp, n)) : nullptr;
    return e->pool.upload(wk);
  };
  const float *w0 = pm.get(pre + "conv0_weight", 64 * 3 * 7 * 7);
  if (!w0 || !fold_bn_f64(pm, pre + "batchnorm0", 64, s, t)) return TN_ERR_MISSING;
  F.stem_w = upload_w(transpose_pad(w0, 64, 147, 160), 160, 64, F.stem_wx);       // (64, 3, 7, 7): k = c * 49 + ky * 7 + kx already
  F.stem_s = e->pool.upload(s); F.stem_t = e->pool.upload(t);
  int outer = 1;
  for (int b = 0; b < 4; ++b) {
    const std::string sp = pre + "stage" + std::to_string(b + 1) + "_";
    for (int l = 0; l < kBlockCfg[b]; ++l) {
      tn_encoder::Fp32Layer L;
      L.cin = e->geom.Cin[b] + 32 * l;
      const float *w1 = pm.get(sp + "conv" + std::to_string(2 * l) + "_weight", (int64_t)128 * L.cin);
      const float *w3 = pm.get(sp + "conv" + std::to_string(2 * l + 1) + "_weight", 32 * 128 * 9);
      if (!w1 || !w3) return TN_ERR_MISSING;
      if (!fold_bn_f64(pm, sp + "batchnorm" + std::to_string(2 * l), L.cin, s, t)) return TN_ERR_MISSING;
      L.s1 = e->pool.upload(s); L.t1 = e->pool.upload(t);
      if (!fold_bn_f64(pm, sp + "batchnorm" + std::to_string(2 * l + 1), 128, s, t)) return TN_ERR_MISSING;
      L.s2 = e->pool.upload(s); L.t2 = e->pool.upload(t);
      L.w1 = upload_w(transpose_pad(w1, 128, L.cin, L.cin), L.cin, 128, L.w1x);
      std::vector<float> w3k((size_t)9 * 128 * 32);
      for (int n = 0; n < 32; ++n)
        for (int c = 0; c < 128; ++c)
          for (int tap = 0; tap < 9; ++tap) w3k[((size_t)tap * 128 + c) * 32 + n] = w3[((size_t)n * 128 + c) * 9 + tap];
      L.w3 = upload_w(w3k, 9 * 128, 32, L.w3x);
      F.layers[b].push_back(L);
    }
    if (b < 3) {
      auto &T = F.trans[b];
      T.cin = e->geom.Cb[b]; T.cout = e->geom.Cb[b] / 2;
      const float *wt = pm.get(pre + "conv" + std::to_string(outer) + "_weight", (int64_t)T.cout * T.cin);
      if (!wt || !fold_bn_f64(pm, pre + "batchnorm" + std::to_string(outer), T.cin, s, t)) return TN_ERR_MISSING;
      T.s = e->pool.upload(s); T.t = e->pool.upload(t);
      T.w = upload_w(transpose_pad(wt, T.cout, T.cin, T.cin), T.cin, T.cout, T.wx);
      ++outer;
    }
  }
  if (!fold_bn_f64(pm, pre + "batchnorm" + std::to_string(outer), e->geom.Cb[3], s, t)) return TN_ERR_MISSING;
  F.head_s = e->pool.upload(s); F.head_t = e->pool.upload(t);

  const size_t weights_bytes = e->pool.bytes;
  e->interleave = getenv("TN_NO_INTERLEAVE") == nullptr && e->split && e->maxB >= 64;     // (two workspace sets, as encoder_run expects)
  const size_t B = (size_t)e->maxB * (e->interleave ? 2 : 1);
  F.stem = (float *)e->pool.alloc(B * e->geom.Hs * e->geom.Ws * 64 * sizeof(float));
  F.bott = (float *)e->pool.alloc(B * e->geom.Hb[0] * e->geom.Wb[0] * 128 * sizeof(float));
  for (int b = 0; b < 4; ++b) F.buf[b] = (float *)e->pool.alloc(B * e->geom.Hb[b] * e->geom.Wb[b] * e->geom.Cb[b] * sizeof(float));
  e->workspace_bytes = e->pool.bytes - weights_bytes;
  if (e->pool.failed) { tn_set_error("device allocation failed"); return TN_ERR_NOMEM; }
  return TN_OK;
}

// Frames [b0, b0 + B) of an fp32-mode encoder, workspace frame slots from w0: stem (BN + ReLU in the epilogue), max pool,
// per dense layer the 1x1 (BN1 + ReLU on load -> raw bottleneck) and the 3x3 (BN2 + ReLU on load -> 32 new channels),
// transitions (BN + ReLU + 2x2 average on load), and the head on the last concat buffer.  An fp32x3 encoder runs the same
// sequence with launch_conv_fp32x3 on the three-term weight images (families "fp32x3_*").
static int encoder_run_range_fp32(tn_encoder *e, const void *x, tn_layout layout, int B, float *feat, hipStream_t s, EventTimer &tm,
                                  int w0, float *cam) {
  auto &F = e->f32;
  int rc;
  const bool x3 = e->fp32x3;
  const std::string mode = x3 ? "fp32x3_" : "fp32_";
  auto launch = [&](const Fp32ConvArgs &a) { return x3 ? launch_conv_fp32x3(a, s) : launch_conv_fp32(a, s); };
  const double fB = (double)B;
  float *stem = F.stem + (size_t)w0 * e->geom.Hs * e->geom.Ws * 64;
  float *bott = F.bott + (size_t)w0 * e->geom.Hb[0] * e->geom.Wb[0] * 128;
  float *buf[4];
  for (int b = 0; b < 4; ++b) buf[b] = F.buf[b] + (size_t)w0 * e->geom.Hb[b] * e->geom.Wb[b] * e->geom.Cb[b];
  const double in_bytes = layout == TN_LAYOUT_NCHW_F32 ? 4 : layout == TN_LAYOUT_NHWC_F16 ? 2 : 1;
  {
    Fp32ConvArgs a{};
    a.kind = FP32_STEM; a.x = x; a.layout = (int)layout; a.K = 147; a.w = F.stem_w; a.wx = F.stem_wx; a.N = 64; a.es = F.stem_s; a.et = F.stem_t;
    a.y = stem; a.ldy = 64; a.M = (long)B * e->geom.Hs * e->geom.Ws; a.H = e->geom.H; a.W = e->geom.W; a.Ho = e->geom.Hs; a.Wo = e->geom.Ws;
    tm.begin((mode + "stem_conv7x7_bn_relu").c_str(), 2.0 * a.M * 64 * 147, fB * e->geom.H * e->geom.W * 3 * in_bytes + a.M * 64 * 4.0);
    rc = launch(a);
    tm.end();
    if (rc) return rc;
    tm.begin((mode + "maxpool3x3s2").c_str(), 0.0, a.M * 64 * 4.0 + fB * e->geom.Hb[0] * e->geom.Wb[0] * 64 * 4);
    rc = launch_maxpool_fp32(stem, B, e->geom.Hs, e->geom.Ws, buf[0], e->geom.Cb[0], e->geom.Hb[0], e->geom.Wb[0], s);
    tm.end();
    if (rc) return rc;
  }
  for (int b = 0; b < 4; ++b) {
    const int Hh = e->geom.Hb[b], Ww = e->geom.Wb[b];
    const long M = (long)B * Hh * Ww;
    const std::string geo = std::to_string(Hh) + "x" + std::to_string(Ww);
    const std::string f1 = mode + "dense1x1_" + geo, f3 = mode + "dense3x3_" + geo;
    for (auto &L : F.layers[b]) {
      Fp32ConvArgs a1{};
      a1.kind = FP32_1X1; a1.x = buf[b]; a1.ldx = e->geom.Cb[b]; a1.K = L.cin; a1.s = L.s1; a1.t = L.t1; a1.w = L.w1; a1.wx = L.w1x; a1.N = 128;
      a1.y = bott; a1.ldy = 128; a1.M = M; a1.H = Hh; a1.W = Ww; a1.Ho = Hh; a1.Wo = Ww;
      tm.begin(f1.c_str(), 2.0 * M * 128 * L.cin, (double)M * (L.cin + 128) * 4 + 128.0 * L.cin * 4);
      rc = launch(a1);
      tm.end();
      if (rc) return rc;
      Fp32ConvArgs a3{};
      a3.kind = FP32_3X3; a3.x = bott; a3.ldx = 128; a3.K = 9 * 128; a3.s = L.s2; a3.t = L.t2; a3.w = L.w3; a3.wx = L.w3x; a3.N = 32;
      a3.y = buf[b]; a3.ldy = e->geom.Cb[b]; a3.yoff = L.cin; a3.M = M; a3.H = Hh; a3.W = Ww; a3.Ho = Hh; a3.Wo = Ww;
      tm.begin(f3.c_str(), 2.0 * M * 32 * 1152, (double)M * (128 + 32) * 4 + 32.0 * 1152 * 4);
      rc = launch(a3);
      tm.end();
      if (rc) return rc;
    }
    if (b < 3) {
      auto &T = F.trans[b];
      Fp32ConvArgs at{};
      at.kind = FP32_TRANS; at.x = buf[b]; at.ldx = e->geom.Cb[b]; at.K = T.cin; at.s = T.s; at.t = T.t; at.w = T.w; at.wx = T.wx; at.N = T.cout;
      at.y = buf[b + 1]; at.ldy = e->geom.Cb[b + 1]; at.M = (long)B * e->geom.Hb[b + 1] * e->geom.Wb[b + 1]; at.H = Hh; at.W = Ww;
      at.Ho = e->geom.Hb[b + 1]; at.Wo = e->geom.Wb[b + 1];
      tm.begin((mode + "transition_" + geo).c_str(), 2.0 * at.M * T.cout * T.cin,
               (double)M * T.cin * 4 + (double)at.M * T.cout * 4 + (double)T.cout * T.cin * 4);
      rc = launch(at);
      tm.end();
      if (rc) return rc;
    }
  }
  tm.begin("head_bnrelu_avgpool7", 0.0, fB * e->geom.Hb[3] * e->geom.Wb[3] * e->geom.Cb[3] * 4 + fB * e->geom.feat_dim * 4);
  rc = launch_head(nullptr, B, e->geom.Hb[3], e->geom.Wb[3], e->geom.Cb[3], F.head_s, F.head_t, feat, e->geom.PH, e->geom.PW, s, buf[3]);
  tm.end();
  if (rc || !cam) return rc;
  tm.begin("class_maps", 2.0 * fB * 49 * e->geom.feat_dim * e->cam_units,
           fB * e->geom.Hb[3] * e->geom.Wb[3] * e->geom.Cb[3] * 4 + fB * e->cam_units * 49 * e->geom.PH * e->geom.PW * 4);
  rc = launch_class_maps(nullptr, buf[3], B, e->geom.Hb[3], e->geom.Wb[3], e->geom.Cb[3], F.head_s, F.head_t, e->cam_w, e->geom.PH, e->geom.PW,
                         e->cam_units, cam, s);
  tm.end();
  return rc;
}

// one layer's folded host parameters as the block kernels' packers take them (Block14Layer and Block7Layer: the same five fields)
struct BlockLayerHost { std::vector<float> w1f, s1, t1, t2; const float *w3; };
template <typename T>
static std::vector<T> block_layers(const std::vector<BlockLayerHost> &hl) {
  std::vector<T> v;
  for (const auto &h : hl) v.push_back(T{h.w1f.data(), h.w3, h.s1.data(), h.t1.data(), h.t2.data()});
  return v;
}

extern "C" int tn_densenet121_create(tn_ctx *ctx, const tn_param *params, int n_params, const char *prefix_c,
                                     int height, int width, int max_batch, tn_encoder **out) {
  return tn_densenet121_create_ex(ctx, params, n_params, prefix_c, height, width, max_batch, 0, out);
}

extern "C" int tn_densenet121_create_ex(tn_ctx *ctx, const tn_param *params, int n_params, const char *prefix_c,
                                        int height, int width, int max_batch, int flags, tn_encoder **out) {
  TN_REQUIRE(ctx && params && out && prefix_c, "tn_densenet121_create: null argument");
  TN_REQUIRE((flags & ~(TN_ENC_EXACT_WEIGHTS | TN_ENC_FP32 | TN_ENC_FP32X3)) == 0, "tn_densenet121_create_ex: unknown flag");
  TN_REQUIRE((flags & (TN_ENC_FP32 | TN_ENC_FP32X3)) != (TN_ENC_FP32 | TN_ENC_FP32X3),
             "tn_densenet121_create_ex: TN_ENC_FP32 and TN_ENC_FP32X3 are two modes, choose one");
  TN_REQUIRE(max_batch > 0, "tn_densenet121_create: max_batch must be positive");
  TN_REQUIRE(height >= 224 && width >= 224 && height <= 1024 && width <= 1024,
             "tn_densenet121_create: input size must be in [224,1024] (AvgPool2D(7) needs a >=7x7 final map)");
  const EncPolicy p = enc_policy(flags);
  const EncGeom g = enc_geom(height, width);
  if (const char *why = enc_refusal(p, g)) { tn_set_error(why); return TN_ERR_INVALID; }
  TN_ON_DEVICE(ctx->device);
  const std::string pre(prefix_c);
  ParamMap pm(params, n_params);
  tn_encoder *e = new tn_encoder();
  e->ctx = ctx;
  e->geom = g; e->policy = p; e->maxB = max_batch; e->last_batch = 0;
  e->split = getenv("TN_NO_SPLIT") == nullptr;
  e->nsplit = getenv("TN_SPLIT") ? atoi(getenv("TN_SPLIT")) : 2;
  if (e->nsplit != 4) e->nsplit = 2;
  e->fp32x3 = (flags & TN_ENC_FP32X3) != 0;
  e->fp32 = (flags & TN_ENC_FP32) != 0 || e->fp32x3;             // (the fp32x3 mode is the fp32 mode's network on another kernel)
  for (int i = 0; i < 4; ++i) {
    if (hipStreamCreateWithFlags(&e->side[i], hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_done[0][i], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_done[1][i], hipEventDisableTiming) != hipSuccess) {
      tn_set_error("could not create the side streams");
      delete e;
      return TN_ERR_HIP;
    }
  }
  if (hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming) != hipSuccess) { tn_set_error("hipEventCreate failed"); delete e; return TN_ERR_HIP; }
  auto fail = [&](int code) { e->pool.release(); delete e; return code; };
  if (e->fp32) {
    const int rc = create_fp32(e, pm, pre);
    if (rc) return fail(rc);
    *out = e;
    return TN_OK;
  }

  std::vector<float> s, t;
  // ---- centred stem output (round 6) ----
  // The pooled stem map is what every dense layer of block 1 and the first transition read, through a BatchNorm each.  Stored
  // as it is, a channel whose values sit many standard deviations from zero loses its information to fp16's RELATIVE precision:
  // the extreme case is a (near-)dead channel of batchnorm0 (gamma ~ 0: the output is the constant relu(beta)), whose
  // consumers normalise with a running variance at the epsilon floor - scale gamma / sqrt(1e-5) = 316 gamma on the rounding
  // error of a constant, 1e-2 on the features of EVERY frame (tests/tools/trained_like.py, scripts/round_study.py).  All of a
  // channel's consumers carry an estimate of its mean, their running_mean; the map is stored as relu(bn(conv)) - m_c with m_c
  // their average, and the constant goes into the consumers' shifts, shift' = shift + scale m_c (exact: no kernel knows).
  e->stem_centre.assign(64, 0.f);
  if (getenv("TN_NO_STEM_CENTRE") == nullptr) {
    std::vector<double> acc(64, 0.0);
    int cnt = 0;
    for (int l = 0; l <= kBlockCfg[0]; ++l) {
      const std::string bn = l < kBlockCfg[0] ? pre + "stage1_batchnorm" + std::to_string(2 * l) : pre + "batchnorm1";
      const float *mu = pm.get(bn + "_running_mean", l < kBlockCfg[0] ? 64 + 32 * l : 64 + 32 * kBlockCfg[0]);
      if (!mu) return fail(TN_ERR_MISSING);
      for (int c = 0; c < 64; ++c) acc[c] += mu[c];
      ++cnt;
    }
    for (int c = 0; c < 64; ++c) {
      const float m = (float)(acc[c] / cnt);
      e->stem_centre[c] = std::isfinite(m) ? m : 0.f;
    }
  }
  auto centre_shift = [&](std::vector<float> &sc, std::vector<float> &sh) {       // a consumer of block 1's channels 0 .. 63
    for (int c = 0; c < 64; ++c) sh[c] = (float)((double)sh[c] + (double)sc[c] * (double)e->stem_centre[c]);
  };
  {  // stem: conv0 + batchnorm0 (fold_stem, above)
    const float *w0 = pm.get(pre + "conv0_weight", 64 * 3 * 7 * 7);
    if (!w0 || !fold_bn(pm, pre + "batchnorm0", 64, s, t)) return fail(TN_ERR_MISSING);
    const StemFold f = fold_stem(w0, s.data(), t.data(), e->stem_centre.data(), p.exact);
    e->stem_wp = e->pool.upload(f.wp);
    e->stem_wp_zf = e->pool.upload(f.wp_zf);
    if (p.exact) e->stem_wp_zf_lo = e->pool.upload(f.wp_zf_lo);
    e->stem_scale = e->pool.upload(f.scale);
    e->stem_shift = e->pool.upload(f.shift);
    e->stem_shift_u8 = e->pool.upload(f.shift_u8);
    e->stem_floor = e->pool.upload(f.floor);
  }
  e->zeros128 = e->pool.upload(std::vector<float>(128, 0.0f));
  e->ones128 = e->pool.upload(std::vector<float>(128, 1.0f));
  int outer = 1;
  for (int b = 0; b < 4; ++b) {
    const std::string sp = pre + "stage" + std::to_string(b + 1) + "_";
    const DenseStreamKernel *sk = enc_stream_kernel(p, g, b);
    const bool block7 = enc_block7(p, g, b);
    std::vector<BlockLayerHost> hl;     // host copies for the block kernels' packers (only where one of them takes the block)
    for (int l = 0; l < kBlockCfg[b]; ++l) {
      tn_encoder::DenseLayer L;
      L.cin = enc_layer_cin(g, b, l);
      const float *w1 = pm.get(sp + "conv" + std::to_string(2 * l) + "_weight", (int64_t)128 * L.cin);
      const float *w3 = pm.get(sp + "conv" + std::to_string(2 * l + 1) + "_weight", 32 * 128 * 9);
      if (!w1 || !w3) return fail(TN_ERR_MISSING);
      if (!fold_bn(pm, sp + "batchnorm" + std::to_string(2 * l), L.cin, s, t)) return fail(TN_ERR_MISSING);
      if (b == 0) centre_shift(s, t);
      // BN1 + ReLU as relu(s x + t) = sw clamp(x, lo, hi) + tc with lo, hi fp16 numbers (calib_host.hip::bn_relu_clamp_fold: no
      // arithmetic and no rounding in front of the 1x1); every kernel of the layer gets (lo, hi) as its constants, sw[k] w[n][k] as
      // its weights and sum_k w[n][k] tc[k] inside BN2's shift
      std::vector<float> sw1(L.cin), tc1(L.cin);
      bn_relu_clamp_fold(std::vector<float>(s).data(), std::vector<float>(t).data(), L.cin, s.data(), t.data(), sw1.data(), tc1.data());
      L.s1 = e->pool.upload(s); L.t1 = e->pool.upload(t);
      // input_means hands out block 1's 1x1 operand means in the reference graph's units, clamp(x_centred, lo, hi) + m_c - except in
      // a channel the fold made a constant (scale 0 / not finite, or a threshold past the fp16 range on the clipped side): its operand
      // is 0 whatever the centring
      if (b == 0)
        for (int c = 0; c < 64; ++c) e->calib_centre.push_back(s[c] != t[c] ? e->stem_centre[c] : 0.f);
      // x0[k] = clamp(0, lo, hi): the operand's value on the CLIPPED side of a channel whose ReLU is off at x = 0 (round 6, below)
      std::vector<float> x0(L.cin);
      for (int k = 0; k < L.cin; ++k) x0[k] = std::fmin(std::fmax(0.f, s[k]), t[k]);
      if (sk || block7) hl.push_back(BlockLayerHost{{}, s, t, {}, w3});
      // The scale of the BatchNorm BEHIND the 1x1 convolution is folded into its weights before they are rounded to fp16
      // (or split into hi + lo): bn2(conv(a)) = conv'(a) + shift with w'[n][k] = scale[n] w[n][k].  That is how the fp16
      // model is defined (weights.as_fp16_model hands over w with scale[n] w[n][k] fp16-representable); the kernels that
      // still apply a scale get ones.
      if (!fold_bn(pm, sp + "batchnorm" + std::to_string(2 * l + 1), 128, s, t)) return fail(TN_ERR_MISSING);
      std::vector<float> w1f((size_t)128 * L.cin);
      bool in_range = true;
      // The constant of the clamp form, sum_k w[n][k] tc[k], is computed here in double from the exact weights, while the matrix
      // pipe multiplies the ROUNDED folded weight with clamp(x).  On the clipped side of a channel the two have to cancel
      // (sw lo + tc = 0), and they only do so to the precision of the rounded weight times |lo|: a near-dead BatchNorm channel
      // with a negative shift (scale 1e-5, threshold 1e4, folded weight in fp16's subnormals) left 3e-4 per weight that way
      // (scripts/dead_debug.py: 4.8e-3 on the features in the exact-weights mode).  Round 6: the operand is split at
      // x0 = clamp(0, lo, hi) - sw clamp(x) + tc = sw (clamp(x) - x0) + (tc + sw x0) - and the x0 part of the matrix product is
      // taken out of the shift with the SAME rounded weights the pipe uses: what is left of a weight's rounding error multiplies
      // clamp(x) - x0 (zero on the clipped side), what the exact weights multiply is tc + sw x0 (= s (x0 - c): no cancellation).
      for (int n = 0; n < 128; ++n) {
        double bias = 0.0, corr = 0.0;
        for (int k = 0; k < L.cin; ++k) {
          const float wf = s[n] * sw1[k] * w1[(size_t)n * L.cin + k];
          w1f[(size_t)n * L.cin + k] = wf;
          in_range = in_range && std::fabs(wf) <= 65504.0f;
          bias += (double)w1[(size_t)n * L.cin + k] * ((double)tc1[k] + (double)sw1[k] * (double)x0[k]);
          if (x0[k] != 0.f) {
            const float hi = (float)(f16)wf;
            const double weff = p.exact ? (double)hi + (double)(float)(f16)(wf - hi) : (double)hi;      // what the kernels multiply (split_hi_lo_rows / to_f16)
            corr += weff * (double)x0[k];
          }
        }
        t[n] = (float)((double)t[n] + (double)s[n] * bias - corr);
      }
      if (!in_range) { tn_set_error("a 1x1 weight leaves the fp16 range once its BatchNorm scales are folded in (" + sp + "conv" + std::to_string(2 * l) + ")"); return fail(TN_ERR_INVALID); }
      if (p.exact) {
        const int bk = enc_exact_ktile(p, g, b, l);
        L.w1 = e->pool.upload(split_hi_lo_rows(w1f.data(), 128, L.cin, (L.cin + bk - 1) / bk * bk));
      } else {
        L.w1 = e->pool.upload(to_f16(w1f.data(), (size_t)128 * L.cin));
      }
      if (sk || block7) { hl.back().w1f = w1f; hl.back().t2 = t; }
      if (enc_layer_strip(p, g, b, l)) L.w1s = e->pool.upload(pack_w1_strip(w1f.data(), L.cin, t.data()));
      L.s2 = e->pool.upload(std::vector<float>(128, 1.0f)); L.t2 = e->pool.upload(t);
      if (p.exact) {       // packed image of hi, then packed image of lo
        std::vector<float> hi(32 * 128 * 9), lo(32 * 128 * 9);
        for (size_t i = 0; i < hi.size(); ++i) {
          hi[i] = (float)(f16)w3[i];
          lo[i] = w3[i] - hi[i];
        }
        std::vector<f16> img = pack_conv3x3(hi.data());
        const std::vector<f16> img_lo = pack_conv3x3(lo.data());
        img.insert(img.end(), img_lo.begin(), img_lo.end());
        L.w3p = e->pool.upload(img);
      } else {
        L.w3p = e->pool.upload(pack_conv3x3(w3));
      }
      if (L.w1s) L.w3s = e->pool.upload(pack_w3_strip(w3));
      e->layers[b].push_back(L);
    }
    if (sk) {
      DenseStreamArgs &as = e->b_stream[b];
      as.stream = e->pool.upload(sk->pack(block_layers<Block14Layer>(hl), g.Cin[b]));
      as.total_units = sk->units(g.Cin[b], kBlockCfg[b]);
      as.ldc = g.Cb[b]; as.K0 = g.Cin[b]; as.nl = kBlockCfg[b];
    } else if (block7) {
      const Block7Image img = pack_block7(block_layers<Block7Layer>(hl), g.Cin[b]);
      DenseBlock7Args &a7 = e->b7[b];
      a7.wa = e->pool.upload(img.wa); a7.wb = e->pool.upload(img.wb); a7.tab = e->pool.upload(img.tab);
      for (int w = 0; w < 4; ++w) { a7.a_off[w] = img.a_off[w]; a7.b_off[w] = img.b_off[w]; }
      a7.ldc = g.Cb[b]; a7.K0 = g.Cin[b]; a7.nl = kBlockCfg[b];
    }
    {
      std::vector<DenseLayerDev> cd;
      for (auto &L : e->layers[b]) cd.push_back(DenseLayerDev{L.s1, L.t1, L.w1, L.s2, L.t2, L.w3p});
      e->chain_dev[b] = e->pool.upload(cd);
    }
    if (const int nl = enc_strip_chain_layers(p, g, b)) {      // the block's leading strip layers as one launch
      std::vector<DenseStripLayerDev> sd;
      for (int l = 0; l < nl; ++l) {
        const auto &L = e->layers[b][l];
        sd.push_back(DenseStripLayerDev{L.s1, L.t1, L.w1s, L.w3s});
      }
      e->strip_chain_dev[b] = e->pool.upload(sd);
    }
    if (b < 3) {
      auto &T = e->trans[b];
      T.cin = g.Cb[b]; T.cout = g.Cb[b] / 2;
      const float *wt = pm.get(pre + "conv" + std::to_string(outer) + "_weight", (int64_t)T.cout * T.cin);
      if (!wt || !fold_bn(pm, pre + "batchnorm" + std::to_string(outer), T.cin, s, t)) return fail(TN_ERR_MISSING);
      if (b == 0) centre_shift(s, t);
      T.s = e->pool.upload(s); T.t = e->pool.upload(t);
      T.w = p.exact ? e->pool.upload(split_hi_lo_rows(wt, T.cout, T.cin, T.cin))
                     : e->pool.upload(to_f16(wt, (size_t)T.cout * T.cin));
      if (!p.exact && (T.cout == 512 || T.cout == 256) && T.cin % 128 == 0) {      // the warp-specialised kernel of the last two transitions (trans_ws.hip decides at launch)
        const std::vector<f16> wh = to_f16(wt, (size_t)T.cout * T.cin);
        T.wfrag = e->pool.upload(pack_trans_frags(wh.data(), T.cout, T.cin));
      }
      ++outer;
    }
  }
  if (!fold_bn(pm, pre + "batchnorm" + std::to_string(outer), g.Cb[3], s, t)) return fail(TN_ERR_MISSING);
  e->head_s = e->pool.upload(s); e->head_t = e->pool.upload(t);

  const size_t weights_bytes = e->pool.bytes;
  // Round 6: with pipelined forwards a batch is no longer cut in two halves that run side by side - consecutive WHOLE batches run
  // side by side on the two side streams (encoder_run), each in its own workspace set: twice the frames per launch
  // (bench.py --batch 512 measured what that is worth before it was built: +2.1 %, the per-launch drain / fill of the chip
  // amortised over two frames per CU).  TN_NO_INTERLEAVE: the half-batch form of rounds 1 - 5.
  e->interleave = getenv("TN_NO_INTERLEAVE") == nullptr && e->split && max_batch >= 64;
  const size_t B = (size_t)max_batch * (e->interleave ? 2 : 1);
  e->stem_out = (f16 *)e->pool.alloc(B * g.Hs * g.Ws * 64 * sizeof(f16));
  e->bott = (f16 *)e->pool.alloc(B * g.Hb[0] * g.Wb[0] * 128 * sizeof(f16));
  for (int b = 0; b < 4; ++b)
    e->blockbuf[b] = (f16 *)e->pool.alloc(B * g.Hb[b] * g.Wb[b] * g.Cb[b] * sizeof(f16));
  if (enc_block7(p, g, 3)) e->head32 = (float *)e->pool.alloc(B * g.Hb[3] * g.Wb[3] * g.Cb[3] * sizeof(float));
  for (int b = 0; b < 4; ++b)
    if (const DenseStreamKernel *sk = enc_stream_kernel(p, g, b)) e->b_stream_scratch[b] = (f16 *)e->pool.alloc(B * sk->scratch_halfs() * sizeof(f16));
  e->workspace_bytes = e->pool.bytes - weights_bytes;
  if (e->pool.failed) { tn_set_error("device allocation failed"); return fail(TN_ERR_NOMEM); }
  // The streamed kernels read the 32 channels a layer is about to write as the zero-weighted pad of its last 64-channel super-step
  // (dense_block28.hip also rows 28 .. 31 of a plane): whatever is there must be finite, so the buffers do not start as whatever
  // the allocator left in them
  for (int b = 0; b < 4; ++b)
    if (const DenseStreamKernel *sk = enc_stream_kernel(p, g, b))
      if (hipMemset(e->blockbuf[b], 0, B * g.Hb[b] * g.Wb[b] * g.Cb[b] * sizeof(f16)) != hipSuccess ||
          hipMemset(e->b_stream_scratch[b], 0, B * sk->scratch_halfs() * sizeof(f16)) != hipSuccess) {
        tn_set_error("hipMemset failed");
        return fail(TN_ERR_HIP);
      }
  *out = e;
  return TN_OK;
}

extern "C" int tn_densenet121_feature_dim(const tn_encoder *enc) { return enc ? enc->geom.feat_dim : 0; }
extern "C" size_t tn_densenet121_workspace_bytes(const tn_encoder *enc) { return enc ? enc->workspace_bytes : 0; }

// Frames [b0, b0+B) of the batch on stream s.  Every buffer is per-frame contiguous, so a
// sub-batch is just a pointer offset; weights are shared read-only.  Which kernel runs which dense layers is the plan's
// decision (encoder_plan.h::enc_block_plan); this function fills the launch arguments of the steps it is given.
static int encoder_run_range(tn_encoder *e, const void *x0, tn_layout layout, int b0, int B, float *feat0,
                             hipStream_t s, EventTimer &tm, int ws0 = -1, bool shared_chip = false) {
  int rc;
  const EncGeom &g = e->geom;
  const EncPolicy &p = e->policy;
  const double fB = (double)B;
  const size_t frame_bytes = (size_t)g.H * g.W * 3 * (layout == TN_LAYOUT_NCHW_F32 ? 4 : layout == TN_LAYOUT_NHWC_F16 ? 2 : 1);
  const void *x = (const unsigned char *)x0 + (size_t)b0 * frame_bytes;
  float *feat = feat0 + (size_t)b0 * g.feat_dim;
  const int w0 = ws0 >= 0 ? ws0 : b0;        // first frame slot of the workspace (the second workspace set starts at maxB)
  // the class activation maps of frames [b0, b0 + B), nullptr outside tn_densenet121_forward_class_maps
  float *cam = e->cam_w ? e->cam_out + (size_t)b0 * e->cam_units * 49 * g.PH * g.PW : nullptr;
  if (e->fp32) return encoder_run_range_fp32(e, x, layout, B, feat, s, tm, w0, cam);
  f16 *stem_out = e->stem_out + (size_t)w0 * g.Hs * g.Ws * 64;
  f16 *bott = e->bott + (size_t)w0 * g.Hb[0] * g.Wb[0] * 128;
  f16 *bbuf[4];
  for (int b = 0; b < 4; ++b) bbuf[b] = e->blockbuf[b] + (size_t)w0 * g.Hb[b] * g.Wb[b] * g.Cb[b];
  // calibration pass (tn_densenet121_input_means): layer-wise kernels only, and behind every BatchNorm + ReLU that feeds a
  // convolution the per-channel mean of that input, in execution order
  const bool cal = e->calib_dev != nullptr;
  float *cal_out = e->calib_dev;
  auto cal_mean = [&](const f16 *xin, int ld, int K, const float *sc, const float *sh, long rows, int clamp = 0) {
    const int rc2 = launch_channel_mean(xin, ld, K, sc, sh, rows, e->calib_scratch, cal_out, s, clamp);
    cal_out += K;
    return rc2;
  };
  std::vector<EncStep> plan[4];
  for (int b = 0; b < 4; ++b) plan[b] = enc_block_plan(p, g, b, B, cal, shared_chip);
  // the head reads the last block un-rounded when the kernels that produce it write the fp32 side copy: the LDS-resident 7x7
  // block kernel and the transition in front of it
  // ... unless they apply the head themselves and write this range's features (round 10): no side copy, no head launch
  const bool head_fused = enc_head_fused(p, g, cal, e->cam_w != nullptr, tm.on) && plan[3][0].route == ENC_BLOCK7;
  float *h32 = !head_fused && plan[3][0].route == ENC_BLOCK7 ? e->head32 + (size_t)w0 * g.Hb[3] * g.Wb[3] * g.Cb[3] : nullptr;
  auto begin = [&](const std::string &family, const EncCost &c) { tm.begin(family.c_str(), c.flops, c.bytes); };
  {
    StemArgs a{x, (int)layout, B, g.H, g.W, e->stem_wp, e->stem_wp_zf, e->stem_scale, e->stem_shift, stem_out, g.Hs, g.Ws};
    a.shift_u8 = e->stem_shift_u8;
    a.wp_zf_lo = e->stem_wp_zf_lo;
    a.floor = e->stem_floor;
    if (p.fuse) {
      begin("stem_conv_bn_relu_maxpool", stem_pool_cost(g, fB));
      rc = launch_stem_pool(a, bbuf[0], g.Cb[0], g.Hb[0], g.Wb[0], s);
      tm.end();
      if (rc) return rc;
    } else {
      begin("stem_conv7x7_bn_relu", stem_cost(g, fB));
      rc = launch_stem(a, s);
      tm.end();
      if (rc) return rc;
      begin("maxpool3x3s2", maxpool_cost(g, fB));
      rc = launch_maxpool3x3s2(stem_out, B, g.Hs, g.Ws, 64, bbuf[0], g.Cb[0], g.Hb[0], g.Wb[0], s);      // (the stem map is centred already: max commutes with the constant)
      tm.end();
      if (rc) return rc;
    }
  }
  for (int b = 0; b < 4; ++b) {
    const int Hh = g.Hb[b], Ww = g.Wb[b];
    const int M = B * Hh * Ww;
    for (const EncStep &st : plan[b]) {
      auto &L = e->layers[b][st.l0];
      if (st.route != ENC_LAYERWISE) begin(family_name(st, g, b), step_cost(st, g, b, M));
      switch (st.route) {
        case ENC_STREAM14:
        case ENC_STREAM28: {
          // pixel-owning waves, all weights streamed through an LDS ring (dense_block14.hip; dense_block28.hip: in four passes of
          // eight rows, the weights streamed once per pass)
          const DenseStreamKernel &sk = kDenseStreamKernels[st.route];
          DenseStreamArgs as = e->b_stream[b];
          as.buf = bbuf[b]; as.B = B;
          as.scratch = e->b_stream_scratch[b] + (size_t)w0 * sk.scratch_halfs();
          rc = sk.launch(as, s);
          break;
        }
        case ENC_BLOCK7: {
          // the frame's concat buffer stays in LDS for the whole block; only the weights stream (dense_block7.hip)
          DenseBlock7Args a7 = e->b7[b];
          a7.buf = bbuf[b]; a7.B = B;
          a7.side = b == 3 ? h32 : nullptr;
          if (b == 3 && head_fused) { a7.feat = feat; a7.head_s = e->head_s; a7.head_t = e->head_t; a7.ldfeat = g.feat_dim; }
          rc = launch_dense_block7(a7, s);
          break;
        }
        case ENC_CHAIN_TILE:      // one workgroup per frame walks the whole block: no launch gaps, no cold prologue per layer
                                  // (28 x 28: layers [l0, l0 + nl) behind the strip layers, chain_dev from entry l0 on)
        case ENC_TILE: {
          const bool ch = st.route == ENC_CHAIN_TILE;
          DenseLayerArgs af{bbuf[b], g.Cb[b], L.cin, L.s1, L.t1, L.w1, L.s2, L.t2, L.w3p, B, Hh, Ww, nullptr, p.dl_variant, ch ? e->chain_dev[b] + st.l0 : nullptr, ch ? st.nl : 0};
          af.exact = p.exact;
          rc = launch_dense_layer(af, s);
          break;
        }
        case ENC_STRIP_CHAIN: {
          DenseStripChainArgs ac{bbuf[b], g.Cb[b], g.Cin[b], st.nl, e->strip_chain_dev[b], B, Hh, Ww};
          rc = st.paired ? launch_dense_strip_pair_chain(ac, s) : launch_dense_strip_chain(ac, s);
          break;
        }
        case ENC_STRIP: {
          DenseStripArgs as{bbuf[b], g.Cb[b], L.cin, L.s1, L.t1, L.w1s, L.w3s, B, Hh, Ww};
          rc = st.paired ? launch_dense_strip_pair(as, s) : launch_dense_strip(as, s);
          break;
        }
        default: {      // ENC_LAYERWISE
          // un-fused: BN2 (scale folded into the weights) adds its shift in the 1x1's epilogue, the 3x3 only applies the ReLU
          // (the 1x1's operand is clamp(x, lo, hi): that is what its folded weights multiply, and what the calibration averages)
          if (cal && (rc = cal_mean(bbuf[b], g.Cb[b], L.cin, L.s1, L.t1, M, 1))) return rc;
          Conv1x1Args a1{bbuf[b], g.Cb[b], L.cin, L.s1, L.t1, L.w1, 128, bott, 128, 0, M, 0, Hh, Ww};
          a1.bias = L.t2;
          a1.clamp = 1;
          a1.exact = p.exact;
          begin(family_name(st, g, b), conv1x1_cost(M, L.cin));
          rc = launch_conv1x1(a1, s);
          tm.end();
          if (rc) return rc;
          if (cal && (rc = cal_mean(bott, 128, 128, e->ones128, e->zeros128, M))) return rc;
          Conv3x3Args a3{bott, L.s2, e->zeros128, L.w3p, bbuf[b], g.Cb[b], L.cin, M, Hh, Ww};
          a3.exact = p.exact;
          begin("conv3x3_bnrelu", conv3x3_cost(M));
          rc = launch_conv3x3(a3, s);
        }
      }
      tm.end();
      if (rc) return rc;
    }
    if (b < 3) {
      auto &T = e->trans[b];
      const int Mo = B * g.Hb[b + 1] * g.Wb[b + 1];
      if (cal && (rc = cal_mean(bbuf[b], g.Cb[b], T.cin, T.s, T.t, M))) return rc;
      Conv1x1Args at{bbuf[b], g.Cb[b], T.cin, T.s, T.t, T.w, T.cout, bbuf[b + 1], g.Cb[b + 1], 0, Mo, 1, Hh, Ww};
      at.exact = p.exact;
      at.wfrag = cal ? nullptr : T.wfrag;
      if (b == 2 && h32) { at.y32 = h32; at.ld32 = g.Cb[3]; }
      if (b == 2 && head_fused) { at.feat = feat; at.head_s = e->head_s; at.head_t = e->head_t; at.ldfeat = g.feat_dim; }
      begin("transition_conv1x1_avgpool", transition_cost(M, Mo, T.cin, T.cout));
      rc = launch_conv1x1(at, s);
      tm.end();
      if (rc) return rc;
    }
  }
  if (head_fused) return TN_OK;      // (the features are written; no class maps on this route)
  begin("head_bnrelu_avgpool7", head_cost(g, fB));
  rc = launch_head(bbuf[3], B, g.Hb[3], g.Wb[3], g.Cb[3], e->head_s, e->head_t, feat, g.PH, g.PW, s, h32);
  tm.end();
  if (rc || !cam) return rc;
  // the same source the head just read (h32 where this forward wrote it), the same BatchNorm + ReLU on load, this range's stream
  tm.begin("class_maps", 2.0 * fB * 49 * g.feat_dim * e->cam_units, fB * g.Hb[3] * g.Wb[3] * g.Cb[3] * (h32 ? 4 : 2) + fB * e->cam_units * 49 * g.PH * g.PW * 4);
  rc = launch_class_maps(bbuf[3], h32, B, g.Hb[3], g.Wb[3], g.Cb[3], e->head_s, e->head_t, e->cam_w, g.PH, g.PW, e->cam_units, cam, s);
  tm.end();
  return rc;
}

static int encoder_run(tn_encoder *e, const void *x, tn_layout layout, int B, float *feat, EventTimer &tm) {
  TN_REQUIRE(e && x && feat, "tn_densenet121_forward: null argument");
  TN_REQUIRE(B > 0 && B <= e->maxB, "tn_densenet121_forward: batch exceeds max_batch");
  TN_ON_DEVICE(e->ctx->device);
  hipStream_t s = e->ctx->stream;
  e->last_batch = B;
  // Large batches run as two half-batches on two side streams: the halves drift apart, so one
  // half's load-bound kernels (56^2 block) overlap the other's MFMA-bound ones (measured +6%).
  // The caller's stream is fenced with events on both sides, so stream order is preserved.
  const int ns = e->nsplit;
  const bool split = e->split && !tm.on && B >= 32 * ns && (B % (8 * ns)) == 0;
  const int par = (int)(e->calls & 1);
  e->calls++;
  e->last_ws0 = 0;
  if (!split) {
    // (a pipelined encoder: earlier calls may still run on the side streams and share the workspace)
    if (e->pipelined) {
      for (int h = 0; h < e->split_of[par ^ 1]; ++h) TN_HIP_CHECK(hipStreamWaitEvent(s, e->ev_done[par ^ 1][h], 0));
      for (int h = 0; h < ns; ++h) TN_HIP_CHECK(hipStreamWaitEvent(s, e->ev_done[par][h], 0));   // (the call before that one)
    }
    e->split_of[par] = 0;
    return encoder_run_range(e, x, layout, 0, B, feat, s, tm);
  }
  if (e->pipelined && e->interleave && B / ns >= e->policy.strip_min_batch) {      // (a batch whose halves would run the small-batch kernels keeps them: one kernel family per batch size, pipelined or not)
    // Whole batch on side stream `par`, workspace set `par`: the call before runs on the other stream in the other set, the
    // call before that was on this stream (stream order separates the two users of a set).  A call of the half-batch form
    // may still be in flight on either stream (the mode was switched, or a small batch came in between): wait for it.
    TN_HIP_CHECK(hipEventRecord(e->ev_in, s));
    TN_HIP_CHECK(hipStreamWaitEvent(e->side[par], e->ev_in, 0));
    if (!e->last_interleaved)
      for (int p2 = 0; p2 < 2; ++p2)
        for (int g = 0; g < e->split_of[p2]; ++g) TN_HIP_CHECK(hipStreamWaitEvent(e->side[par], e->ev_done[p2][g], 0));
    e->last_interleaved = true;
    e->last_ws0 = par * e->maxB;
    // (the one place whose kernels share the chip with the other stream's call: the paired 28x28 strip launches, encoder_plan.h)
    const int r = encoder_run_range(e, x, layout, 0, B, feat, e->side[par], tm, par * e->maxB, true);
    TN_HIP_CHECK(hipEventRecord(e->ev_done[par][0], e->side[par]));
    e->split_of[par] = 1;
    e->split_batch = 0;
    return r;
  }
  if (e->last_interleaved) {      // back to the half-batch form: its row ranges cut across both workspace sets' users
    for (int h = 0; h < ns; ++h)
      for (int p2 = 0; p2 < 2; ++p2)
        for (int g = 0; g < e->split_of[p2]; ++g) TN_HIP_CHECK(hipStreamWaitEvent(e->side[h], e->ev_done[p2][g], 0));
    e->last_interleaved = false;
  }
  TN_HIP_CHECK(hipEventRecord(e->ev_in, s));
  // Pipelined calls overlap on the side streams, and half h of every call works in workspace rows [h B / ns, (h + 1) B / ns):
  // equal batch sizes keep each row range on one stream, whose order then separates consecutive calls.  When the batch size
  // changes (a corpus' ragged last batch) the ranges shift across streams: every side stream first waits for everything the
  // earlier calls left on ANY side stream.
  if (e->pipelined && e->split_batch != 0 && e->split_batch != B) {
    for (int h = 0; h < ns; ++h)
      for (int p2 = 0; p2 < 2; ++p2)
        for (int g = 0; g < e->split_of[p2]; ++g) TN_HIP_CHECK(hipStreamWaitEvent(e->side[h], e->ev_done[p2][g], 0));
  }
  e->split_batch = B;
  int rc = TN_OK;
  for (int h = 0; h < ns; ++h) {
    TN_HIP_CHECK(hipStreamWaitEvent(e->side[h], e->ev_in, 0));
    const int r = encoder_run_range(e, x, layout, h * (B / ns), B / ns, feat, e->side[h], tm);
    if (r) rc = r;
    TN_HIP_CHECK(hipEventRecord(e->ev_done[par][h], e->side[h]));
    // pipelined: the join is the caller's (tn_densenet121_join), so that the next call's first half can start beside
    // the tail of this call's second half (the last chained block of a half batch runs on half of the CUs)
    if (!e->pipelined) TN_HIP_CHECK(hipStreamWaitEvent(s, e->ev_done[par][h], 0));
  }
  e->split_of[par] = ns;
  return rc;
}

static int encoder_join(tn_encoder *e, int lag) {
  if (e->calls - 1 - lag < 0) return TN_OK;
  const int par = (int)((e->calls - 1 - lag) & 1);
  for (int h = 0; h < e->split_of[par]; ++h) TN_HIP_CHECK(hipStreamWaitEvent(e->ctx->stream, e->ev_done[par][h], 0));
  return TN_OK;
}

extern "C" int tn_densenet121_set_pipelined(tn_encoder *enc, int on) {
  TN_REQUIRE(enc, "tn_densenet121_set_pipelined: null handle");
  TN_ON_DEVICE(enc->ctx->device);
  if (enc->pipelined && !on) {            // leaving the mode: everything issued so far is joined
    int rc = encoder_join(enc, 0);
    if (rc == TN_OK) rc = encoder_join(enc, 1);
    if (rc) return rc;
  }
  enc->pipelined = on != 0;
  return TN_OK;
}

extern "C" int tn_densenet121_join(tn_encoder *enc, int lag) {
  TN_REQUIRE(enc, "tn_densenet121_join: null handle");
  TN_REQUIRE(lag == 0 || lag == 1, "tn_densenet121_join: lag must be 0 (the last forward) or 1 (the one before)");
  TN_ON_DEVICE(enc->ctx->device);
  return encoder_join(enc, lag);
}

extern "C" int tn_densenet121_forward(tn_encoder *enc, const void *x, tn_layout layout, int batch, float *feat) {
  EventTimer tm;
  return encoder_run(enc, x, layout, batch, feat, tm);
}

extern "C" int tn_densenet121_class_map_dims(const tn_encoder *enc, int *h, int *w) {
  TN_REQUIRE(enc && h && w, "tn_densenet121_class_map_dims: null argument");
  *h = 7 * enc->geom.PH;
  *w = 7 * enc->geom.PW;
  return TN_OK;
}

// forward with `cam_*` set for the duration of the call: every range launches the maps behind its head (encoder_run_range)
static int class_maps_check(const char *fn, tn_encoder *enc, const void *x, float *feat, const tn_dense *classes, float *maps) {
  const std::string f(fn);
  TN_REQUIRE(enc, f + ": null encoder");
  TN_REQUIRE(x, f + ": x is null");
  TN_REQUIRE(feat, f + ": features is null");
  TN_REQUIRE(classes, f + ": classes is null");
  TN_REQUIRE(maps, f + ": maps is null");
  TN_REQUIRE(classes->ctx == enc->ctx, f + ": classes belongs to another context than the encoder");
  TN_REQUIRE(classes->in_units == enc->geom.feat_dim, f + ": classes has in_units " + std::to_string(classes->in_units) + ", the encoder's feature width is " +
                                                          std::to_string(enc->geom.feat_dim));
  TN_REQUIRE(classes->units <= 64, f + ": classes has " + std::to_string(classes->units) + " units, the maps take at most 64");
  TN_REQUIRE(enc->calib_dev == nullptr, f + ": a calibration pass is in progress");
  return TN_OK;
}

extern "C" int tn_densenet121_forward_class_maps(tn_encoder *enc, const void *x, tn_layout layout, int batch, float *feat,
                                                 const tn_dense *classes, float *maps) {
  if (int rc = class_maps_check("tn_densenet121_forward_class_maps", enc, x, feat, classes, maps)) return rc;
  enc->cam_w = classes->w; enc->cam_out = maps; enc->cam_units = classes->units;
  EventTimer tm;
  const int rc = encoder_run(enc, x, layout, batch, feat, tm);
  enc->cam_w = nullptr; enc->cam_out = nullptr; enc->cam_units = 0;
  return rc;
}

// the same under the event timer (one stream, as tn_densenet121_profile): the family "class_maps" beside "head_bnrelu_avgpool7"
extern "C" int tn_dbg_profile_class_maps(tn_encoder *enc, const void *x, tn_layout layout, int batch, float *feat,
                                                 const tn_dense *classes, float *maps, tn_kernel_stat *stats, int max_stats, int *n_stats) {
  TN_REQUIRE(stats && n_stats, "tn_dbg_profile_class_maps: null argument");
  if (int rc = class_maps_check("tn_dbg_profile_class_maps", enc, x, feat, classes, maps)) return rc;
  enc->cam_w = classes->w; enc->cam_out = maps; enc->cam_units = classes->units;
  EventTimer tm;
  tm.on = true;
  tm.s = enc->ctx->stream;
  const int rc = encoder_run(enc, x, layout, batch, feat, tm);
  tm.finish();
  enc->cam_w = nullptr; enc->cam_out = nullptr; enc->cam_units = 0;
  if (rc) return rc;
  const int n = (int)tm.fams.size() < max_stats ? (int)tm.fams.size() : max_stats;
  for (int i = 0; i < n; ++i) stats[i] = tm.fams[i];
  *n_stats = n;
  return TN_OK;
}

extern "C" int tn_densenet121_profile(tn_encoder *enc, const void *x, tn_layout layout, int batch, float *feat,
                                      tn_kernel_stat *stats, int max_stats, int *n_stats) {
  TN_REQUIRE(enc && stats && n_stats, "tn_densenet121_profile: null argument");
  EventTimer tm;
  tm.on = true;
  tm.s = enc->ctx->stream;
  const int rc = encoder_run(enc, x, layout, batch, feat, tm);
  tm.finish();
  if (rc) return rc;
  const int n = (int)tm.fams.size() < max_stats ? (int)tm.fams.size() : max_stats;
  for (int i = 0; i < n; ++i) stats[i] = tm.fams[i];
  *n_stats = n;
  return TN_OK;
}

// Calibration statistics for weights.as_fp16_model(input_means=...): runs `batch` frames through the LAYER-WISE kernels and
// returns, for the 119 convolutions behind the stem in execution order (per dense layer: the 1x1's K inputs, then the 3x3's
// 128; a transition's inputs behind its block), the per-input-channel mean of the activation the convolution reads.
extern "C" int tn_densenet121_input_means(tn_encoder *e, const void *x, tn_layout layout, int batch, float *means_host,
                                          int64_t capacity, int64_t *numel) {
  TN_REQUIRE(e && x && means_host && numel, "tn_densenet121_input_means: null argument");
  TN_REQUIRE(batch > 0 && batch <= e->maxB, "tn_densenet121_input_means: batch exceeds max_batch");
  TN_REQUIRE(!e->fp32x3, "tn_densenet121_input_means: not for an fp32x3-mode encoder (TN_ENC_FP32X3: no fp16 conversion to calibrate)");
  TN_REQUIRE(!e->fp32, "tn_densenet121_input_means: not for an fp32-mode encoder (TN_ENC_FP32: no fp16 conversion to calibrate)");
  TN_REQUIRE(!e->policy.exact, "tn_densenet121_input_means: not for an exact-weights encoder");
  TN_ON_DEVICE(e->ctx->device);
  int64_t n = 0;
  for (int b = 0; b < 4; ++b) {
    for (auto &L : e->layers[b]) n += L.cin + 128;
    if (b < 3) n += e->trans[b].cin;
  }
  *numel = n;
  TN_REQUIRE(capacity >= n, "tn_densenet121_input_means: host buffer too small");
  if (int rc = encoder_join(e, 0)) return rc;
  if (int rc = encoder_join(e, 1)) return rc;     // (the call before the last one may still run, in the workspace set this pass uses)
  hipStream_t s = e->ctx->stream;
  float *dev = nullptr, *feat = nullptr;
  double *scratch = nullptr;
  auto release = [&]() { (void)hipFree(dev); (void)hipFree(feat); (void)hipFree(scratch); e->calib_dev = nullptr; e->calib_scratch = nullptr; };
  if (hipMalloc((void **)&dev, sizeof(float) * n) != hipSuccess || hipMalloc((void **)&feat, sizeof(float) * (size_t)batch * e->geom.feat_dim) != hipSuccess ||
      hipMalloc((void **)&scratch, sizeof(double) * 32 * 1024) != hipSuccess) {
    release();
    tn_set_error("tn_densenet121_input_means: device allocation failed");
    return TN_ERR_NOMEM;
  }
  e->calib_dev = dev; e->calib_scratch = scratch;
  EventTimer tm;
  int rc = encoder_run_range(e, x, layout, 0, batch, feat, s, tm);
  if (!rc && hipMemcpyAsync(means_host, dev, sizeof(float) * n, hipMemcpyDeviceToHost, s) != hipSuccess) rc = TN_ERR_HIP;
  if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = TN_ERR_HIP;
  if (!rc) {      // block 1's 1x1 operands are clamps of the CENTRED stem channels: hand out the means in the reference graph's units
    int64_t o = 0;
    for (size_t l = 0; l < e->layers[0].size(); ++l) {
      for (int c = 0; c < 64; ++c) means_host[o + c] += e->calib_centre[l * 64 + c];
      o += e->layers[0][l].cin + 128;
    }
  }
  release();
  if (rc == TN_ERR_HIP) tn_set_error("tn_densenet121_input_means: HIP error");
  e->last_batch = batch;
  e->last_ws0 = 0;      // (the pass ran in workspace set 0: read_tap reads its frames, not those of a pipelined forward in set 1)
  return rc;
}

extern "C" int tn_densenet121_read_tap(tn_encoder *e, const char *tap_c, int batch, float *out_host, size_t capacity,
                                       size_t *numel) {
  TN_REQUIRE(e && tap_c && out_host && numel, "tn_densenet121_read_tap: null argument");
  TN_REQUIRE(!e->fp32x3, "read_tap: not for an fp32x3-mode encoder (TN_ENC_FP32X3: its maps are fp32, the taps hand out fp16 maps)");
  TN_REQUIRE(!e->fp32, "read_tap: not for an fp32-mode encoder (TN_ENC_FP32: its maps are fp32, the taps hand out fp16 maps)");
  TN_REQUIRE(batch > 0 && batch <= e->last_batch, "tn_densenet121_read_tap: batch exceeds the last forward");
  const std::string tap(tap_c);
  const f16 *src = nullptr;
  int hh = 0, ww = 0, cc = 0, ld = 0;
  if (tap == "stem") {
    TN_REQUIRE(!e->policy.fuse, "read_tap: the stem map is not materialised when stem+maxpool are fused (use pool0)");
    src = e->stem_out; hh = e->geom.Hs; ww = e->geom.Ws; cc = 64; ld = 64;
  }
  else if (tap == "pool0") { src = e->blockbuf[0]; hh = e->geom.Hb[0]; ww = e->geom.Wb[0]; cc = 64; ld = e->geom.Cb[0]; }
  else if (tap.rfind("stage", 0) == 0 && tap.size() == 6) {
    const int b = tap[5] - '1';
    TN_REQUIRE(b >= 0 && b < 4, "read_tap: bad stage");
    src = e->blockbuf[b]; hh = e->geom.Hb[b]; ww = e->geom.Wb[b]; cc = e->geom.Cb[b]; ld = cc;
  } else if (tap.rfind("trans", 0) == 0 && tap.size() == 6) {
    const int b = tap[5] - '1';
    TN_REQUIRE(b >= 0 && b < 3, "read_tap: bad transition");
    src = e->blockbuf[b + 1]; hh = e->geom.Hb[b + 1]; ww = e->geom.Wb[b + 1]; cc = e->geom.Cb[b] / 2; ld = e->geom.Cb[b + 1];
  } else {
    TN_REQUIRE(false, "read_tap: unknown tap");
  }
  const size_t px = (size_t)batch * hh * ww;
  *numel = px * cc;
  TN_REQUIRE(capacity >= *numel, "read_tap: host buffer too small");
  src += (size_t)e->last_ws0 * hh * ww * ld;      // (the workspace set the last forward ran in)
  if (int rc = encoder_join(e, 0)) return rc;
  if (int rc = encoder_join(e, 1)) return rc;
  TN_HIP_CHECK(hipStreamSynchronize(e->ctx->stream));
  std::vector<f16> tmp(px * ld);
  TN_HIP_CHECK(hipMemcpy(tmp.data(), src, tmp.size() * sizeof(f16), hipMemcpyDeviceToHost));
  // (the stem's output is stored centred: the tap hands out the values the reference's graph has)
  const bool centred = tap == "stem" || tap == "pool0" || tap == "stage1";
  for (size_t p = 0; p < px; ++p)
    for (int c = 0; c < cc; ++c) out_host[p * cc + c] = (float)tmp[p * ld + c] + (centred && c < 64 ? e->stem_centre[c] : 0.f);
  return TN_OK;
}

extern "C" int tn_densenet121_destroy(tn_encoder *enc) {
  if (!enc) return TN_OK;
  TnDeviceGuard tn_dg_(enc->ctx->device);
  for (int i = 0; i < 4; ++i) { (void)hipStreamSynchronize(enc->side[i]); (void)hipStreamDestroy(enc->side[i]); (void)hipEventDestroy(enc->ev_done[0][i]); (void)hipEventDestroy(enc->ev_done[1][i]); }
  (void)hipEventDestroy(enc->ev_in);
  enc->pool.release();
  delete enc;
  return TN_OK;
}
