// Fused DenseNet dense layer, "strip-streaming" form (round 3; 56x56 and 28x28 blocks, K <= 320):
//
//   y[.., K:K+32] = conv3x3( relu(bn2( conv1x1( relu(bn1( x[.., 0:K] )) ) )) )
//
// (reference call site models/vision/definitions.py:30 -> gluoncv DenseNet _make_dense_layer: BatchNorm-Activation-
// Conv1x1-BatchNorm-Activation-Conv3x3-Concat).  dense_layer_big.hip owns ROUT image rows per 8-wave workgroup and runs its
// phases (K loop, epilogue, 3x3, store) one after the other behind barriers, with the bottleneck tile in LDS aliasing the
// K-loop ring.  This kernel is built the other way round:
//
// * a workgroup = one frame, 4 waves = ONE wave per SIMD with the whole 512-entry register file; no barrier after the
//   prologue.  A wave owns a pair of adjacent 14-pixel column strips (2 x 16 slots with their halo columns = the N = 32 of
//   one v_mfma_f32_32x32x16_f16) and walks DOWN its rows one image row at a time.  One wave per SIMD issues one instruction
//   per ~4 cycles: a 32-cycle 32x32x16 MFMA hides ~6 other instructions, a 16-cycle 16x16x32 only one
//   (scripts/microbench/slotbench.hip) - and this layer needs ~3.5 element-wise / LDS / load instructions per 16x16x32's worth
//   of MFMA work, so the kernel is built on the 32x32 shape.
// * the 128-channel bottleneck never touches LDS: with the weights as the A operand, the accumulator layout of the 1x1 GEMM
//   (lane = slot l & 31, rows (r & 3) + 8 (r >> 2) + 4 (l >> 5)) IS the B-operand layout of the 3x3's MFMAs once the 3x3
//   weights are packed with the matching permutation of their input channels (chained MFMAs: BN2 + ReLU + fp16 pack are
//   lane-local).  The sliding window of three bottleneck rows lives in 96 literal accumulator registers.
// * the 3x3 convolution applies the three kernel columns to the SAME input fragment into three accumulator sets which are
//   combined at the end by two DPP row shifts: out[x] = acc[dx=0][x] + acc[dx=-1][x-1] + acc[dx=+1][x+1].  The shifts stay
//   inside the 16-lane row = inside one strip (outputs of the halo slots are never stored): no cross-fragment carry.
// * the layer's 1x1 weights (K x 128, as A fragments) and all nine taps of the 3x3 weights (72 KB) are resident in LDS for
//   the whole launch; activations go HBM -> registers directly in fragment shape (64 B per lane per 64-channel super-step;
//   the two lanes of a pixel cover one 128-B line) through a register ring that holds one whole row and is refilled with
//   the next row as it is read out.
// * BN2 costs no element-wise multiply-add: its scale is folded into the 1x1 weights on the host (before the fp16 rounding:
//   the fp16 model is DEFINED that way, weights.as_fp16_model) and its shift enters the GEMM through one extra 16-channel
//   k-step whose pixel fragment is the constant (1, 1, m, 0, ...): weight columns shift_hi, shift_lo (two fp16 numbers = 22
//   bits of the fp32 shift) and 1; m = -60000 in the lanes of padding columns, so that their ReLU'd bottleneck is 0 as
//   the convolution's zero padding demands.  What is left of epilogue A is convert + ReLU + the window write.
// * the schedule is pinned by hand: the body is a sequence of SLOTS - one MFMA followed by its share of everything else -
//   with a scheduling barrier behind each.  1x1 slots carry BN1 + ReLU of the next k-step, the weight-fragment and constant
//   reads, the ring refill and the DPP epilogue of the PREVIOUS output row; 3x3 slots carry the weight-fragment reload, the
//   BN2 epilogue of the row just computed (its window row is only needed by the last third of the slots) and the first
//   operands of the next row.  Nothing runs outside an MFMA's shadow in the steady state.
//
// No halo recompute in y at 56x56 beyond one row per wave (29 / 28); 16 / 14 in x.
#include <array>
#include <type_traits>

#pragma once
#include "common.h"

#ifndef TN_DS_EXP
#define TN_DS_EXP 0   // timing experiments only (results wrong): bit 0 no activation loads inside the row loop, bit 1 no 3x3 phase, bit 2 no 1x1 phase, bit 3 / 4 no weight-fragment reads in the 3x3 / 1x1 phase
#endif

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2_t __attribute__((ext_vector_type(2)));

constexpr int kW3Bytes = 3 * 8 * 3 * 1024;   // [dy][k16-step][dx] fragments of 1 KiB

template <int W, int KS>
struct DSGeom {
  // A frame = NPAIR strip pairs (28 columns each; the last pair of a width that is no multiple of 28 is partly empty) x NCHUNK
  // row chunks of ROWS output rows = NITEM work items, one per wave, four per workgroup: 56 x 56 and 28 x 28 frames are one
  // workgroup (2 x 2 and 1 x 4 items); the 128 x 128 / 64 x 64 maps of a 512 x 512 input take 5 x 4 = 20 / 3 x 4 = 12 items =
  // 5 / 3 workgroups per frame.  A chunk recomputes the bottleneck row above and below it.
  static constexpr int NPAIR = (W + 27) / 28;    // strip pairs per frame
  static constexpr int ROWS = W == 56 ? 28 : W == 28 ? 7 : W / 4;     // output rows per wave
  static constexpr int NCHUNK = W / ROWS;
  static constexpr int NITEM = NPAIR * NCHUNK, WGS = NITEM / 4;       // workgroups per frame
  static constexpr int FPW = 1;                  // frames per workgroup (2: DSGeomPair)
  static constexpr int KQ = 2 * KS;              // 16-channel k-steps
  static constexpr int NSU = (KS + 1) / 2;       // 64-channel super-steps (the last one is half when KS is odd)
  static constexpr int W1OFF = kW3Bytes;                   // KQ + 1 k-steps of 4 fragments: the last one carries BN2's shift
  static constexpr int T1OFF = W1OFF + (KQ + 1) * 4096;    // a1[K] | b1[K] (fp16: BN1 as v_pk_fma_f16, csrc/calib_host.hip)
  static constexpr int LDS_BYTES = T1OFF + KS * 32 * 4;
  static_assert(W % ROWS == 0 && NITEM % 4 == 0 && ROWS >= 4, "strip geometry");
  static_assert(NSU <= 5, "the activation ring holds five super-steps");
  static_assert(LDS_BYTES <= 160 * 1024, "weights do not fit LDS");
};

// The 28 x 28 frame in the paired form (dense_strip_pair_w28.hip): TWO frames per workgroup, each wave walks half a frame - 14 output
// rows, twice as many as a quarter to spread the per-wave fill (weight prologue, cold first row, window warm-up, exposed last
// epilogue) over, and 15 or 16 bottleneck rows for them where two quarters compute 17 or 18.  Wave w: frame 2 blockIdx.x + (w >> 1),
// rows [14 (w & 1), + 14).  LDS map, slot schedules and window registers are DSGeom<28, KS>'s; the layer's weights serve both frames.
template <int KS>
struct DSGeomPair : DSGeom<28, KS> {
  static constexpr int ROWS = 14, NCHUNK = 2, NITEM = 2, WGS = 1, FPW = 2;
};

// The bottleneck window lives in LITERAL accumulator registers a[160:255] (three rows x eight 16-channel k-steps x one
// 4-register MFMA B operand): hipcc's MFMA builtin takes A / B from VGPRs only, and a window held in compiler-allocated AGPR
// values gets its live ranges split and copied through VGPRs (measured in the first version: ~200 extra v_accvgpr moves per
// row group, some of them directly in front of the asm MFMA that reads the register two cycles later - a hazard hipcc cannot
// see).  Every slot of the kernel body names all 96 registers as clobbered, which keeps compiler values out of them;
// scripts/audit_strip_isa.py checks the ISA for strays (cdna_hip_programming.md 5.7 item 4).
#define TN_WIN_BASE 160
#define TN_WIN_CLOBBER                                                                                                              \
  "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175",   \
  "a176", "a177", "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191",   \
  "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207",   \
  "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222", "a223",   \
  "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237", "a238", "a239",   \
  "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252", "a253", "a254", "a255"
constexpr int win_reg(int prow, int t) { return TN_WIN_BASE + 32 * prow + 4 * t; }
// keeps compiler values that are live here out of the window registers (no instruction)
#define TN_WIN_FENCE() asm volatile("" ::: TN_WIN_CLOBBER)

// four packed VGPRs -> window tuple (physical row PROW, k-step T).  v_accvgpr_write -> MFMA operand read needs two wait states:
// the schedule puts at least eight slots between the write of a tuple and the first MFMA that reads it
template <int PROW, int T>
__device__ __forceinline__ void win_write(const unsigned v0, const unsigned v1, const unsigned v2, const unsigned v3) {
  constexpr int B = win_reg(PROW, T);
  asm volatile("v_accvgpr_write_b32 a%c4, %0\n\tv_accvgpr_write_b32 a%c5, %1\n\tv_accvgpr_write_b32 a%c6, %2\n\tv_accvgpr_write_b32 a%c7, %3"
               :: "v"(v0), "v"(v1), "v"(v2), "v"(v3), "n"(B), "n"(B + 1), "n"(B + 2), "n"(B + 3) : TN_WIN_CLOBBER);
}
template <int R>
__device__ __forceinline__ void win_zero_reg() {
  asm volatile("v_accvgpr_write_b32 a%c0, 0" :: "n"(R) : TN_WIN_CLOBBER);
}
// a bottleneck row above / below the image: zeros
template <int PROW>
__device__ __forceinline__ void win_zero() {
  [&]<int... I>(std::integer_sequence<int, I...>) { (win_zero_reg<win_reg(PROW, 0) + I>(), ...); }(std::make_integer_sequence<int, 32>{});
  asm volatile("s_nop 1");
}
// one 3x3 weight fragment against window tuple (PROW, T)
template <bool FIRST, int PROW, int T>
__device__ __forceinline__ void mfma32_win(f32x16 &d, const u32x4 a) {
  constexpr int B0 = win_reg(PROW, T);
  if constexpr (FIRST)
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, a[%c2:%c3], 0" : "=&a"(d) : "v"(a), "n"(B0), "n"(B0 + 3));
  else
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, a[%c2:%c3], %0" : "+a"(d) : "v"(a), "n"(B0), "n"(B0 + 3));
}
// The LAST k-step of a 3x3 phase: its three MFMAs (one per kernel column) and the wait states their results need before
// anything but an MFMA of the same chain may read them, in ONE statement.  hipcc knows nothing about the latency of an asm
// MFMA: where the accumulators change registers at a control-flow join it put v_accvgpr_mov copies four instructions behind
// the last MFMA, in front of the wait states the consumer carried (round 3, the 128 x 128 geometry: registers 14 / 15 of every
// accumulator - the last pass of the MFMA - copied too early; which instantiations get such copies is the register
// allocator's choice).  With the wait inside the producing statement no copy can come between.
template <int PROW, int T>
__device__ __forceinline__ void mfma32_win_last3(f32x16 &d0, f32x16 &d1, f32x16 &d2, const u32x4 a0, const u32x4 a1, const u32x4 a2) {
  constexpr int B0 = win_reg(PROW, T);
  asm volatile("v_mfma_f32_32x32x16_f16 %0, %3, a[%c6:%c7], %0\n\tv_mfma_f32_32x32x16_f16 %1, %4, a[%c6:%c7], %1\n\t"
               "v_mfma_f32_32x32x16_f16 %2, %5, a[%c6:%c7], %2\n\ts_nop 15\n\ts_nop 3"
               : "+a"(d0), "+a"(d1), "+a"(d2) : "v"(a0), "v"(a1), "v"(a2), "n"(B0), "n"(B0 + 3));
}
__device__ __forceinline__ f32x16 mfma32(const u32x4 a, const u32x4 b, const f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

#define TN_INL __attribute__((always_inline))
template <int N, typename F>
__device__ __forceinline__ void static_for(F &&f) {
  [&]<int... I>(std::integer_sequence<int, I...>) TN_INL { (f(std::integral_constant<int, I>{}), ...); }(std::make_integer_sequence<int, N>{});
}
template <int V>
using ic = std::integral_constant<int, V>;

#define TN_SB() __builtin_amdgcn_sched_barrier(0)

// One LDS-DMA piece: 64 lanes x 16 B, global (per-lane address) -> LDS (wave-uniform base in M0 + lane * 16).  Inline asm:
// hipcc treats the builtin as an LDS store and orders every later ds_read behind a vmcnt(0) (dense_layer_big.hip).
__device__ __forceinline__ void dma16(const void *gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_dst)
               : "memory");
}

// ---- the static schedule ----
struct PItem { int kind, q, j; };     // kind: 0 none, 1 C(q), 2 BN(q).j, 3 LD(u = q).i = j
template <int KS>
struct PList { PItem it[7 * 2 * KS + 8]; int n; };
template <int KS>
constexpr PList<KS> make_pl() {
  constexpr int KQ = 2 * KS, NSU = (KS + 1) / 2;
  constexpr bool ODD = (KS & 1) != 0;
  PList<KS> l{};
  int n = 0;
  for (int c = 0; c < 3 && c < KQ; ++c) l.it[n++] = PItem{1, c, 0};
  for (int q = 0; q < KQ; ++q) {
    for (int j = 0; j < 4; ++j) l.it[n++] = PItem{2, q, j};
    if (q + 3 < KQ) l.it[n++] = PItem{1, q + 3, 0};
    const int u = q >> 2;
    const bool half = ODD && u == NSU - 1;
    if (half ? (q & 3) == 1 : (q & 3) == 3)
      for (int i = 0; i < (half ? 2 : 4); ++i) l.it[n++] = PItem{3, u, i};
  }
  l.n = n;
  return l;
}
template <int KS>
inline constexpr PList<KS> kPL = make_pl<KS>();
template <int KS>
constexpr PItem pl_at(int idx) { return idx >= 0 && idx < kPL<KS>.n ? kPL<KS>.it[idx] : PItem{0, 0, 0}; }
template <int KS>
constexpr int pl_len() { return kPL<KS>.n; }
constexpr int kPLB = 30;                 // pipeline items that run in the previous row's 3x3 phase (slots 42 - 71)
constexpr int kXN = 8;                   // pixel-fragment buffers
struct ASlot { int pl0, npl, epb0, nepb; };
template <int N> struct ASched { ASlot s[N]; };
// 1x1 slot i (k-step i / 4): pipeline items [pl0, pl0 + npl) and epilogue B items [epb0, epb0 + nepb).  The items left are
// spread evenly over the slots left; BN(q) has to be complete when k-step q starts, so the pipeline goes first whenever it is
// needed within the current k-step, otherwise the epilogue B items (24) are used up first.
template <int KS>
constexpr auto make_a_sched() {
  constexpr int KQ = 2 * KS, NA = 4 * (KQ + 1), NPL = pl_len<KS>();
  ASched<NA> r{};
  int bn3[KQ + 1] = {};                                   // index of BN(q).3 in the list
  for (int i = 0; i < NPL; ++i)
    if (kPL<KS>.it[i].kind == 2 && kPL<KS>.it[i].j == 3) bn3[kPL<KS>.it[i].q] = i;
  int pos = NPL < kPLB ? NPL : kPLB, epb = 0;
  for (int i = 0; i < NA; ++i) {
    const int qn = i / 4 + 1, rem = 3 - i % 4;          // next k-step, slots left in this one behind slot i
    const int need_end = qn < KQ ? bn3[qn] + 1 : 0;
    const int left = NA - i, total = (NPL - pos) + (24 - epb);
    int quota = (total + left - 1) / left;
    int must = need_end - rem - pos;                    // items the pipeline has to run in this slot not to fall behind
    if (must < 0) must = 0;
    if (must > NPL - pos) must = NPL - pos;
    int npl = must;
    if (quota < npl) quota = npl;
    int ne = 24 - epb < quota - npl ? 24 - epb : quota - npl;
    const int more = NPL - pos - npl < quota - npl - ne ? NPL - pos - npl : quota - npl - ne;
    npl += more;
    r.s[i] = ASlot{pos, npl, epb, ne};
    pos += npl;
    epb += ne;
  }
  return r;
}
template <int KS>
constexpr bool a_sched_complete() {        // every epilogue B item and every pipeline item has a slot
  constexpr int KQ = 2 * KS, NA = 4 * (KQ + 1);
  constexpr auto sa = make_a_sched<KS>();
  int npl = pl_len<KS>() < kPLB ? pl_len<KS>() : kPLB, nepb = 0;
  for (int i = 0; i < NA; ++i) { npl += sa.s[i].npl; nepb += sa.s[i].nepb; }
  return npl == pl_len<KS>() && nepb == 24;
}

template <int W, int KS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void dense_strip_kernel(DenseStripArgs a) {
#define TN_STRIP_TID threadIdx.x
#define TN_STRIP_GEOM DSGeom<W, KS>
#include "dense_strip_body.h"
#undef TN_STRIP_GEOM
#undef TN_STRIP_TID
}

// One layer on the workgroup's frame: one link of the chained kernel (dense_strip_kernel_chain below).  `tid_in`: threadIdx.x
// (the chained kernel hands every layer a copy the compiler cannot see through, so that no per-lane value of one layer stays
// live into the next).
template <int W, int KS>
__device__ __forceinline__ void dense_strip_layer(const DenseStripArgs &a, const int tid_in) {
#define TN_STRIP_TID tid_in
#define TN_STRIP_GEOM DSGeom<W, KS>
#include "dense_strip_body.h"
#undef TN_STRIP_GEOM
#undef TN_STRIP_TID
}


// ---- the block's strip layers as ONE launch (56 x 56 and 28 x 28: a workgroup is one whole frame) ----
// Layer l + 1 of a frame reads nothing but what layers <= l of the SAME frame = the same workgroup wrote: the grid-wide order a
// kernel boundary imposes orders nothing that needs ordering, and costs the drain of the chip, a dispatch and a cold weight
// prologue behind it per layer.  Here the workgroup runs the layer bodies one behind the other, straight-line (every body is its
// own instantiation with its own static schedule; nothing but the argument table is live from one to the next).
template <int W>
struct DSChain {
  static_assert(W == 56 || W == 28, "strip chaining needs one workgroup per frame");
  // K = 64 ... 192 (the first block's first five layers) / K = 128 ... 288 (the second block's first six).  The last layer of
  // the 56 x 56 block, K = 224, stays a launch of its own so that a batch on the timed path still reports the per-layer family
  // dense_layer_strip_56x56 in the instrumented pass: tests/tools/parity_timed.py tells the timed path by that name, and a
  // name may only be reported for a launch that ran.  The seventh strip layer of
  // the 28 x 28 block, K = 320, stays a launch of its own: its body fills the register file exactly when it is compiled alone
  // (256 VGPRs, no spill), and as the seventh link of this kernel hipcc spills five VGPRs of loop-invariant row offsets to
  // scratch (with the thread index handed over opaquely, see below; eleven without).  The six-layer chain has no scratch.
  static constexpr int KS0 = W == 56 ? 2 : 4;
  static constexpr int NL = W == 56 ? 5 : 6;
  static constexpr int LDS_BYTES = DSGeom<W, KS0 + NL - 1>::LDS_BYTES;
};

// Between two layers of a frame.  Layer l + 1 reads (a) LDS that layer l's waves may still be reading - the next weight prologue
// writes over it - and (b) the 32 channels every wave of layer l stored, halo rows / columns of OTHER waves' strips included.
//   * s_waitcnt vmcnt(0): stores count in vmcnt on gfx9, so behind it this wave's stores have been acknowledged by the cache
//     hierarchy; lgkmcnt(0): its LDS reads have returned.  Then ONE workgroup barrier: that holds for all four waves.
//   * Nothing of the next layer is issued ahead of the barrier - its LDS-DMA prologue and its first ring loads are the next
//     statements in program order behind an asm volatile with a memory clobber, a scheduling barrier on either side.
//   * The stale half line: layer l wrote 64 bytes of a 128-byte line whose other half (channels of layer l - 1) an earlier layer
//     of this launch has read through this CU's vector L1.  The L1 is write-through and shared by the CU's waves, and a store
//     goes THROUGH it: it does not leave an older copy of the line behind that a later load of the same CU could hit (the
//     AMDGPU memory model asks of a workgroup-scope release / acquire on gfx942 / gfx950 - not in threadgroup-split mode -
//     exactly the vmcnt(0) wait and nothing else, no buffer_inv).  dense_layer_big.hip's CHAIN and dense_block14.hip rest on the
//     same rule with the same 64-of-128-byte pattern.  What WOULD defeat it is a load that may be served from somewhere the
//     store does not pass: the scalar cache (the ring loads are per-lane vector loads: global_load_dwordx4), or another CU
//     (never: one frame, one workgroup).  The strip's loads and stores carry no cache bits (no sc0 / sc1 / nt), so there is
//     nothing to change on the chained instantiation.
__device__ __forceinline__ void strip_layer_boundary() {
  TN_SB();
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  TN_SB();
}

template <int W>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void dense_strip_kernel_chain(DenseStripChainArgs c) {
  using C = DSChain<W>;
  static_for<C::NL>([&](auto l_tag) TN_INL {
    constexpr int L = decltype(l_tag)::value;
    const DenseStripLayerDev d = c.layers[L];
    const DenseStripArgs a{c.buf, c.ldc, (C::KS0 + L) * 32, d.s1, d.t1, d.w1s, d.w3s, c.B, W, W, nullptr};
    // The lane geometry (pixel column, byte offsets, store masks) is the same in every layer; computed once and kept, it is a
    // dozen VGPRs too many for the widest bodies, which fill the register file on their own: every layer derives its own.
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    __builtin_assume(tid >= 0 && tid < 256);
    dense_strip_layer<W, C::KS0 + L>(a, tid);
    if constexpr (L + 1 < C::NL) strip_layer_boundary();
  });
}

template <int W>
int launch_strip_chain(const DenseStripChainArgs &c, hipStream_t s) {
  using C = DSChain<W>;
  TN_REQUIRE(c.K0 == C::KS0 * 32 && c.nl == C::NL, "dense_strip_chain: not the layer sequence the kernel was built for");
  TN_SET_ATTR_ONCE_PER_DEVICE(TN_HIP_CHECK(hipFuncSetAttribute((const void *)dense_strip_kernel_chain<W>, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES)));
  hipLaunchKernelGGL((dense_strip_kernel_chain<W>), dim3(c.B), dim3(256), C::LDS_BYTES, s, c);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

template <int W, int KS>
int launch_strip(const DenseStripArgs &a, hipStream_t s) {
  using G = DSGeom<W, KS>;
  TN_SET_ATTR_ONCE_PER_DEVICE(TN_HIP_CHECK(hipFuncSetAttribute((const void *)dense_strip_kernel<W, KS>, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS_BYTES)));
  hipLaunchKernelGGL((dense_strip_kernel<W, KS>), dim3(a.B * G::WGS), dim3(256), G::LDS_BYTES, s, a);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

template <int W>
int launch_strip_w(const DenseStripArgs &a, hipStream_t s) {
  switch (a.K / 32) {
    case 2: return launch_strip<W, 2>(a, s);
    case 3: return launch_strip<W, 3>(a, s);
    case 4: return launch_strip<W, 4>(a, s);
    case 5: return launch_strip<W, 5>(a, s);
    case 6: return launch_strip<W, 6>(a, s);
    case 7: return launch_strip<W, 7>(a, s);
    case 8: return launch_strip<W, 8>(a, s);
    case 9: return launch_strip<W, 9>(a, s);
    case 10:
      if constexpr (W != 128) return launch_strip<W, 10>(a, s);     // (W = 128: K <= 288, dense_strip_supported)
      break;
  }
  TN_REQUIRE(false, "dense_strip: K out of range");
}

}  // namespace
