// The routing plan of the fp16 DenseNet-121 encoder: which kernel runs which dense layers, stated once.  tn_densenet121_create
// packs what the predicates below ask for, encoder_run_range launches the steps of enc_block_plan, and tn_dbg_encoder_plan
// (dbg.hip) answers for both without a device.  Host code only: nothing here makes a HIP call.  (The fp32 and fp32x3 modes
// have one route and are not planned; they share EncGeom.)
//
// Precedence inside a block, first match wins (docs/kernels.md "Routes of the dense blocks"):
//   streamed 14x14 / 28x28 block > LDS-resident 7x7 block > chained tile-kernel block >
//   (chained strip launch for the leading layers, then per layer: strip > fused tile kernel > layer-wise 1x1 + 3x3;
//    28x28 at 128 frames or more: the tile-kernel layers behind the strip layers as one chained tile-kernel launch)
// A 28x28 strip step (chained or per layer) of a call that shares the chip with the neighbouring stream's call takes the paired launch
// geometry (EncStep::paired): the same route, family, flops and bytes - the same arithmetic, two frames per workgroup.
#pragma once
#include <cstdlib>
#include <string>
#include <vector>

#include "common.h"

inline constexpr int kBlockCfg[4] = {6, 12, 24, 16};

// ---- the switches (environment and create flags) ----------------------------------------------------------------------------
struct EncPolicy {
  bool fuse = true;            // fused kernels (TN_NO_FUSE: stem, max pool, 1x1 and 3x3 as kernels of their own)
  bool chain = true;           // whole-frame blocks (14x14, 7x7) run all their layers in one launch (TN_NO_CHAIN disables)
  bool chain28 = true;         // the tile-kernel layers of a 28x28 block (K > 320) run in one launch (TN_NO_CHAIN28 or TN_NO_CHAIN: one per layer)
  int chain28_min_batch = 128; // ... from this many frames per launch on (one workgroup per frame, where the per-layer launches spread two
                               // tiles per frame: below it the chained launch leaves more than half of the CUs without work)
  bool exact = false;          // TN_ENC_EXACT_WEIGHTS: dense-layer and transition weights as hi + lo fp16 pairs
  bool strip = true;           // 56x56 / 28x28 layers with K <= 320 run on the strip-streaming kernel (TN_NO_STRIP disables)
  bool strip_chain = true;     // the leading strip layers of a 56x56 / 28x28 block run in one launch (TN_NO_STRIP_CHAIN: one launch per layer)
  int strip_min_batch = 64;    // ... from this many frames per launch on (one workgroup per frame: small batches leave CUs idle)
  bool strip_pair = true;      // the 28x28 strip launches of a call that shares the chip with the neighbouring stream's take two frames per
                               // workgroup, 14 rows per wave (dense_strip_pair_w28.hip; TN_NO_STRIP_PAIR disables)
  int strip_pair_min_batch = 256;  // ... from this many frames per call on (B / 2 workgroups: the neighbour's launch has to take the other half
                                   // of the CUs) and for an even batch (TN_STRIP_PAIR_MIN_BATCH)
  bool block7 = true;          // a 7x7 block runs on the LDS-resident kernel of dense_block7.hip (TN_NO_BLOCK7 disables)
  bool trans_ws = true;        // the last two transitions run on the warp-specialised kernel of trans_ws.hip (TN_NO_TRANS_WS disables; read
                               // by conv1x1.hip's launcher too, which makes the choice)
  bool head_fuse = true;       // the last transition and the 7x7 block kernel apply the head themselves and write the features: no fp32
                               // side copy, no head launch (enc_head_fused; TN_NO_HEAD_FUSE disables)
  // the streamed block kernels (kDenseStreamKernels, common.h): [0] a 14x14 block on dense_block14.hip (TN_NO_BLOCK14 disables),
  // [1] a 28x28 block on dense_block28.hip (TN_BLOCK28=1 enables: measured, not the default)
  bool block_stream[2] = {true, false};
  int dl_variant = 0;          // tuning hook: TN_DL_VARIANT -> DenseLayerArgs.variant
};
static_assert(sizeof(kDenseStreamKernels) / sizeof(kDenseStreamKernels[0]) == 2 && kDenseStreamKernels[0].H == 14 && kDenseStreamKernels[1].H == 28,
              "block_stream[] is indexed like kDenseStreamKernels");

// the one place that reads these switches from the environment
inline EncPolicy enc_policy(int flags) {
  EncPolicy p;
  const bool fp32 = (flags & (TN_ENC_FP32 | TN_ENC_FP32X3)) != 0;
  p.fuse = getenv("TN_NO_FUSE") == nullptr;
  p.chain = getenv("TN_NO_CHAIN") == nullptr;   // measured: -20% on the 14x14 / 7x7 blocks, +2.8% end to end
  p.exact = (flags & TN_ENC_EXACT_WEIGHTS) != 0 && !fp32;    // (TN_ENC_FP32 / TN_ENC_FP32X3 | TN_ENC_EXACT_WEIGHTS: that mode)
  p.strip = getenv("TN_NO_STRIP") == nullptr && !p.exact && p.fuse;
  p.strip_chain = getenv("TN_NO_STRIP_CHAIN") == nullptr;
  p.chain28 = p.chain && getenv("TN_NO_CHAIN28") == nullptr;
  if (getenv("TN_CHAIN28_MIN_BATCH")) p.chain28_min_batch = atoi(getenv("TN_CHAIN28_MIN_BATCH"));
  if (getenv("TN_STRIP_MIN_BATCH")) p.strip_min_batch = atoi(getenv("TN_STRIP_MIN_BATCH"));
  p.strip_pair = getenv("TN_NO_STRIP_PAIR") == nullptr;
  if (getenv("TN_STRIP_PAIR_MIN_BATCH")) p.strip_pair_min_batch = atoi(getenv("TN_STRIP_PAIR_MIN_BATCH"));
  p.block7 = getenv("TN_NO_BLOCK7") == nullptr;
  p.trans_ws = getenv("TN_NO_TRANS_WS") == nullptr;
  p.head_fuse = getenv("TN_NO_HEAD_FUSE") == nullptr;
  p.block_stream[0] = getenv("TN_NO_BLOCK14") == nullptr;
  p.block_stream[1] = getenv("TN_BLOCK28") != nullptr && atoi(getenv("TN_BLOCK28")) != 0;
  p.dl_variant = getenv("TN_DL_VARIANT") ? atoi(getenv("TN_DL_VARIANT")) : 0;
  return p;
}

// ---- the maps of an input size --------------------------------------------------------------------------------------------------
struct EncGeom {
  int H, W;                // input frame
  int Hs, Ws;              // stem conv output
  int Hb[4], Wb[4];        // dense block spatial sizes
  int Cin[4], Cb[4];       // block input / total channels
  int PH, PW, feat_dim;    // AvgPool2D(7) output and the feature vector
};
inline EncGeom enc_geom(int height, int width) {
  EncGeom g;
  g.H = height; g.W = width;
  g.Hs = (height + 6 - 7) / 2 + 1; g.Ws = (width + 6 - 7) / 2 + 1;
  int h = (g.Hs + 2 - 3) / 2 + 1, w = (g.Ws + 2 - 3) / 2 + 1, c = 64;
  for (int b = 0; b < 4; ++b) {
    g.Hb[b] = h; g.Wb[b] = w; g.Cin[b] = c; g.Cb[b] = c + 32 * kBlockCfg[b];
    c = g.Cb[b] / 2; h /= 2; w /= 2;
  }
  g.PH = g.Hb[3] / 7; g.PW = g.Wb[3] / 7;
  g.feat_dim = g.Cb[3] * g.PH * g.PW;
  return g;
}
// what create refuses behind the [224, 1024] range of the input size (nullptr: nothing)
inline const char *enc_refusal(const EncPolicy &p, const EncGeom &g) {
  if (g.PH < 1 || g.PW < 1) return "input too small for AvgPool2D(7)";
  if (g.Wb[0] > 240) return "input too wide for the conv3x3 LDS tile";
  // the hi + lo weight passes: the 8-wave fused layer, the transition kernel and (round 6) the un-fused layer kernels
  if (p.exact && !(p.fuse && (p.dl_variant & ~256) == 0)) return "TN_ENC_EXACT_WEIGHTS needs the default kernels (no TN_NO_FUSE, no TN_DL_VARIANT)";
  return nullptr;
}

// ---- packing predicates: what create packs, and what a route may therefore use ------------------------------------------------
inline int enc_layer_cin(const EncGeom &g, int b, int l) { return g.Cin[b] + 32 * l; }

// the first enabled streamed kernel that supports the block: 14x14, then 28x28 (nullptr: none)
inline const DenseStreamKernel *enc_stream_kernel(const EncPolicy &p, const EncGeom &g, int b) {
  for (const DenseStreamKernel &k : kDenseStreamKernels)
    if (p.fuse && p.block_stream[&k - kDenseStreamKernels] && !p.exact && k.supported(g.Hb[b], g.Wb[b], g.Cin[b], kBlockCfg[b])) return &k;
  return nullptr;
}
// the block's operands are packed for the LDS-resident 7x7 kernel
inline bool enc_block7(const EncPolicy &p, const EncGeom &g, int b) {
  return !enc_stream_kernel(p, g, b) && p.fuse && p.block7 && !p.exact && dense_block7_supported(g.Hb[b], g.Wb[b], g.Cin[b], kBlockCfg[b]);
}
// the layer gets the strip kernel's fragment images
inline bool enc_layer_strip(const EncPolicy &p, const EncGeom &g, int b, int l) {
  return p.strip && dense_strip_supported(g.Hb[b], g.Wb[b], enc_layer_cin(g, b, l));
}
// how many leading layers the chained strip launch takes (0: none): the sequence the chained kernel of the map was built for,
// all of it packed for the strip kernel
inline int enc_strip_chain_layers(const EncPolicy &p, const EncGeom &g, int b) {
  if (!p.strip_chain) return 0;
  const int nl = dense_strip_chain_layers(g.Hb[b], g.Wb[b], g.Cin[b]);
  if (nl <= 0 || nl > kBlockCfg[b]) return 0;
  for (int l = 0; l < nl; ++l)
    if (!enc_layer_strip(p, g, b, l)) return 0;
  return nl;
}
// a fused tile kernel (dense_layer_big.hip) tiles the map and holds the layer's K
inline bool enc_layer_tile(const EncPolicy &p, const EncGeom &g, int b, int l) {
  return p.fuse && dense_layer_supported(g.Hb[b], g.Wb[b]) && enc_layer_cin(g, b, l) <= dense_layer_kmax(g.Wb[b]);
}
// exact mode: the k-tile of the kernel that will run the layer (the row pitch of [hi | lo] is twice K rounded up to it): the
// fused kernel's (64 channels at 14 x 14 and 7 x 7, 32 elsewhere), or conv1x1.hip's 64 where the layer runs layer-wise
inline int enc_exact_ktile(const EncPolicy &p, const EncGeom &g, int b, int l) {
  return !enc_layer_tile(p, g, b, l) ? 64 : (g.Hb[b] == 14 || g.Hb[b] == 7) ? 64 : 32;
}
// one workgroup per frame walks the whole block on the tile kernel (needs no packing of its own)
inline bool enc_block_chained_tile(const EncPolicy &p, const EncGeom &g, int b) {
  const int Hh = g.Hb[b], Ww = g.Wb[b];
  return p.chain && (p.dl_variant & ~(32 | 64 | 128 | 256 | 512)) == 0 && Hh == Ww && (Hh == 14 || Hh == 7 || Hh == 16) &&
         enc_layer_tile(p, g, b, kBlockCfg[b] - 1);
}
// the tile-kernel layers [l0, n) of a 28 x 28 block as one chained launch (dense_layer_kernel<28, 14, 512, 32, 2, true>: one workgroup
// per frame walks layer by layer over the frame's two row tiles): the default fp16 kernels only, every layer from l0 on a tile-kernel
// layer, at least two of them, and the first one at K >= 64 (the two 32-channel k-tiles the kernel requests ahead of a layer's stores).
// Needs no packing of its own: the chain's DenseLayerDev table is the block's chain_dev from entry l0 on.
inline bool enc_chain28(const EncPolicy &p, const EncGeom &g, int b, int l0) {
  if (!p.chain28 || p.exact || p.dl_variant != 0 || g.Hb[b] != 28 || g.Wb[b] != 28) return false;
  if (kBlockCfg[b] - l0 < 2 || enc_layer_cin(g, b, l0) < 64) return false;
  for (int l = l0; l < kBlockCfg[b]; ++l)
    if (!enc_layer_tile(p, g, b, l)) return false;
  return true;
}

// ---- the plan -------------------------------------------------------------------------------------------------------------------
enum EncRoute { ENC_STREAM14, ENC_STREAM28, ENC_BLOCK7, ENC_CHAIN_TILE, ENC_STRIP_CHAIN, ENC_STRIP, ENC_TILE, ENC_LAYERWISE, ENC_NROUTES };
// the family a route's launches are profiled under: the whole name, or (geo) a prefix in front of the block's "HxW"
struct EncRouteName { const char *name; bool geo; };
inline constexpr EncRouteName kEncRouteNames[] = {
    {kDenseStreamKernels[0].family, false}, {kDenseStreamKernels[1].family, false}, {"dense_block_lds_7x7", false},
    {"dense_block_chained_", true}, {"dense_block_strip_", true}, {"dense_layer_strip_", true}, {"dense_layer_fused_", true},
    {"conv1x1_bnrelu", false},      // (layer-wise: and "conv3x3_bnrelu" behind it)
};
static_assert(sizeof(kEncRouteNames) / sizeof(kEncRouteNames[0]) == ENC_NROUTES && ENC_STREAM14 == 0 && ENC_STREAM28 == 1,
              "kEncRouteNames is indexed by EncRoute, whose first two values index kDenseStreamKernels");

// layers [l0, l0 + nl) of the block in one launch (layer-wise: two).  paired: a 28x28 strip step in the two-frames-per-workgroup
// launch geometry (enc_strip_pair)
struct EncStep { EncRoute route; int l0, nl; bool paired = false; };

inline std::string family_name(const EncStep &st, const EncGeom &g, int b) {
  const EncRouteName &n = kEncRouteNames[st.route];
  return n.geo ? n.name + std::to_string(g.Hb[b]) + "x" + std::to_string(g.Wb[b]) : std::string(n.name);
}

// The 28x28 strip steps of the block take the paired launch: only where the call's kernels share the chip with a neighbouring
// stream's (shared_chip: a launch of B / 2 workgroups fills half of the CUs and the neighbour's takes the rest; anywhere else those
// CUs would stand idle), from strip_pair_min_batch frames on, for an even batch (a workgroup takes two frames), and under the
// conditions the strip routes carry themselves: the default fp16 kernels, no tuning variant, not calibrating.
inline bool enc_strip_pair(const EncPolicy &p, const EncGeom &g, int b, int B, bool cal, bool shared_chip) {
  return shared_chip && p.strip_pair && p.strip && !p.exact && p.dl_variant == 0 && !cal && g.Hb[b] == 28 && g.Wb[b] == 28 &&
         B >= p.strip_pair_min_batch && B % 2 == 0;
}

// The head folded into its two producers (round 10): the last transition (trans_ws.hip, the 64 x 512 tile whose 49 rows are the whole
// 7 x 7 frame) writes features 0 .. 511 and the LDS-resident 7x7 block kernel features 512 .. 1023, each from the un-rounded values
// it holds; the fp32 side copy and the head launch fall away.  Only where both producers are those kernels: block 3 on ENC_BLOCK7, the
// transition in the warp-specialised form with N = 512 on a 14 x 14 map, one 7 x 7 pooling window; not when calibrating (layer-wise
// kernels), not for tn_densenet121_forward_class_maps (class_maps: the maps are made from the side copy) and not in the instrumented
// pass (timed: it reports the head family from a launch of its own).  Independent of the batch, of shared_chip and of pipelining.
inline bool enc_head_fused(const EncPolicy &p, const EncGeom &g, bool cal, bool class_maps, bool timed) {
  if (!p.head_fuse || cal || class_maps || timed) return false;
  if (p.dl_variant != 0 || !enc_block7(p, g, 3)) return false;                       // (enc_block_plan: block 3 is {ENC_BLOCK7})
  if (g.Hb[3] != 7 || g.Wb[3] != 7 || g.PH != 1 || g.PW != 1) return false;
  // the transition: what create packs wfrag for and trans_ws_supported accepts, at N = 512 with the frame as one tile
  return p.trans_ws && !p.exact && g.Cb[2] / 2 == 512 && g.Cb[2] % 128 == 0 && g.Hb[2] == 14 && g.Wb[2] == 14;
}

// The launches of block b for a batch of B frames, in order.  cal: the calibration pass (tn_densenet121_input_means), layer-wise
// whatever the switches.  A tuning variant (TN_DL_VARIANT) keeps the block on the tile kernels it tunes.  shared_chip: the call runs
// beside the neighbouring stream's call (encoder_run's interleaved whole-batch branch and nowhere else).
inline std::vector<EncStep> enc_block_plan(const EncPolicy &p, const EncGeom &g, int b, int B, bool cal, bool shared_chip) {
  const int n = kBlockCfg[b], Hh = g.Hb[b];
  std::vector<EncStep> plan;
  if (cal) {
    for (int l = 0; l < n; ++l) plan.push_back({ENC_LAYERWISE, l, 1});
    return plan;
  }
  const bool tuned = p.dl_variant != 0;
  const bool paired = enc_strip_pair(p, g, b, B, cal, shared_chip);
  if (const DenseStreamKernel *sk = tuned ? nullptr : enc_stream_kernel(p, g, b)) return {{(EncRoute)(sk - kDenseStreamKernels), 0, n}};
  if (!tuned && enc_block7(p, g, b)) return {{ENC_BLOCK7, 0, n}};
  if (enc_block_chained_tile(p, g, b)) return {{ENC_CHAIN_TILE, 0, n}};
  // where the per-layer strip route would be taken for the block's leading layers: those layers in one launch (one workgroup
  // per frame walks them; no drain of the chip, no dispatch and no cold start per layer).  The rest follows layer by layer.
  int l = !tuned && B >= p.strip_min_batch ? enc_strip_chain_layers(p, g, b) : 0;
  if (l > 0) plan.push_back({ENC_STRIP_CHAIN, 0, l, paired});
  // (one workgroup per 56 x 56 / 28 x 28 frame, 5 / 3 per 128 x 128 / 64 x 64 frame: enough of them to fill the chip?)
  const bool strip_fills = B * (Hh == 128 ? 5 : Hh == 64 ? 3 : 1) >= p.strip_min_batch;
  for (; l < n; ++l) {
    const EncRoute r = !tuned && strip_fills && enc_layer_strip(p, g, b, l) ? ENC_STRIP : enc_layer_tile(p, g, b, l) ? ENC_TILE : ENC_LAYERWISE;
    // behind the strip layers of a 28 x 28 block: the rest of the block, all of it tile-kernel layers, in one launch (a threshold
    // of its own: one workgroup per frame fills the chip from 128 frames on, together with the neighbouring stream's call)
    if (r == ENC_TILE && B >= p.chain28_min_batch && enc_chain28(p, g, b, l)) {
      plan.push_back({ENC_CHAIN_TILE, l, n - l});
      break;
    }
    plan.push_back({r, l, 1, r == ENC_STRIP && paired});
  }
  return plan;
}

// ---- flops and bytes of a launch, as tn_densenet121_profile reports them ------------------------------------------------------
struct EncCost { double flops = 0, bytes = 0; };
// one dense layer on any fused route (M pixels, cin input channels)
inline EncCost layer_cost(int M, int cin) { return {2.0 * M * (128.0 * cin + 32.0 * 1152), (double)M * (cin + 32) * 2 + 128.0 * cin * 2 + 32.0 * 1152 * 2}; }
// a step of the plan: its layers summed in order (a whole block, or its first layers, under one family name)
inline EncCost step_cost(const EncStep &st, const EncGeom &g, int b, int M) {
  EncCost c;
  for (int l = st.l0; l < st.l0 + st.nl; ++l) {
    const EncCost one = layer_cost(M, enc_layer_cin(g, b, l));
    c.flops += one.flops; c.bytes += one.bytes;
  }
  return c;
}
inline EncCost conv1x1_cost(int M, int cin) { return {2.0 * M * 128.0 * cin, (double)M * (cin + 128) * 2 + 128.0 * cin * 2}; }
inline EncCost conv3x3_cost(int M) { return {2.0 * M * 32.0 * 1152, (double)M * (128 + 32) * 2 + 32.0 * 1152 * 2}; }
inline EncCost transition_cost(int M, int Mo, int cin, int cout) {
  return {2.0 * M * (double)cout * cin, (double)M * cin * 2 + (double)Mo * cout * 2 + (double)cout * cin * 2};
}
// the stem (px: its output pixels) fused with the max pool, on its own, and the max pool; the head
inline EncCost stem_pool_cost(const EncGeom &g, double fB) { return {2.0 * (fB * g.Hs * g.Ws) * 64 * 147, fB * g.H * g.W * 3 * 2 + fB * g.Hb[0] * g.Wb[0] * 64 * 2}; }
inline EncCost stem_cost(const EncGeom &g, double fB) { return {2.0 * (fB * g.Hs * g.Ws) * 64 * 147, fB * g.H * g.W * 3 * 2 + (fB * g.Hs * g.Ws) * 64 * 2}; }
inline EncCost maxpool_cost(const EncGeom &g, double fB) { return {0.0, (fB * g.Hs * g.Ws) * 64 * 2 + fB * g.Hb[0] * g.Wb[0] * 64 * 2}; }
inline EncCost head_cost(const EncGeom &g, double fB) { return {0.0, fB * g.Hb[3] * g.Wb[3] * g.Cb[3] * 2 + fB * g.feat_dim * 4}; }
