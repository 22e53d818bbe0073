// What the two "streamed block" kernels, dense_block14.hip and dense_block28.hip, share (included by those two files only; their
// header comments are the design record): pixel-owning waves, ALL weights as one linear stream of 16.5 KiB units through an LDS-DMA
// ring of kNR slots, activations through a register ring in v[192:255], every steady-state load inline asm with a hand-counted
// s_waitcnt vmcnt(N).  Here: the unit layout and constants, the helpers, a few of the statements between the slots, the host-side
// unit writers and the launcher.  The intervals (su_interval, b_interval) are still written out in each kernel file; tests/tools/
// vmcnt_replay.py models the issue order of BOTH copies and reads the constants from this text plus the kernel's;
// scripts/audit_block14_isa.py checks both kernels' listings for compiler instructions that touch the ring registers.
//
// A kernel built on this core supplies: its per-lane geometry (voff[], the tile addresses), its LDS layout (where the unit ring
// starts), the order of its intervals with the refill targets of each, its prologue and epilogue B - and the host packer that
// writes the units in exactly the order its intervals consume them (StreamWriter below writes one unit; the ORDER is the kernel's).
#pragma once
#include <array>
#include <type_traits>
#include <utility>
#include <vector>

#include "common.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2_t __attribute__((ext_vector_type(2)));

constexpr int kUnitFrag = 16384;                  // 16 A fragments of 1 KiB
constexpr int kUnitBytes = kUnitFrag + 512;       // + BN1 constants of the unit's k-steps: [k-step][lane >> 5][dword J: s[2J], s[2J+1], t[2J], t[2J+1]] fp32
constexpr int kNR = 5;                            // ring slots

// s_waitcnt vmcnt(N) constants (asm loads only; tests/test_cpu_block14.py and tests/test_cpu_block28.py derive every one of them
// from the issue order).  The constants of intervals only one kernel has, or has differently (kVmDmaTail, kVmDmaB0), are in its file.
constexpr int kVmRing = 24;        // a ring register pair is waited for two super-step intervals (2 x 13 loads) after its refills, at the slot of
                                   // the FIRST of its two loads' k-step: 26 - 2 loads lie behind the second one (25 was one too many: the replay test)
constexpr int kVmDmaSU0 = 12, kVmDmaSU = 20, kVmDmaB = 10;

#define TN_INL __attribute__((always_inline))
template <int N, typename F>
__device__ __forceinline__ void static_for(F &&f) {
  [&]<int... I>(std::integer_sequence<int, I...>) TN_INL { (f(std::integral_constant<int, I>{}), ...); }(std::make_integer_sequence<int, N>{});
}
template <int V>
using ic = std::integral_constant<int, V>;
#define TN_SB() __builtin_amdgcn_sched_barrier(0)

__device__ __forceinline__ f32x16 mfma32(const u32x4 a, const u32x4 b, const f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

// LDS-DMA: global (wave-uniform base in SGPRs + per-lane 32-bit offset) -> LDS (M0 + lane * size).  The instruction offset
// applies to the global AND the LDS address (scripts/microbench/dmaoff.hip), so two 1-KiB pieces share one M0.
template <int OFF>
__device__ __forceinline__ void dma16x2(const void *gbase, unsigned voff16, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3 offset:%c4\n\t"
               "global_load_lds_dwordx4 %2, %3 offset:%c5\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "s"(lds_dst), "v"(voff16), "s"(gbase), "n"(OFF), "n"(OFF + 1024));
}
__device__ __forceinline__ void dma4(const void *gbase, unsigned voff4, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %2, %3\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "s"(lds_dst), "v"(voff4), "s"(gbase));
}
template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%c0)" ::"n"(N) : "memory"); }

// The activation ring lives in LITERAL registers v[192:255]: its loads are in flight for two super-step intervals, and a value
// hipcc knows about may be copied or spilled at any time - with the bytes of a pending load not there yet (the first version of
// the 14x14 kernel, ring in compiler-allocated registers tied through the waits: "scratch_store_dwordx4 v[28:31]" one instruction
// behind the load that fills v[28:31]).  Every slot names the 64 registers as clobbered, which keeps compiler values out of them
// (the technique of the strip kernel's accumulator window); scripts/audit_block14_isa.py checks the ISA for strays.
#define TN_RING_BASE 192
#define TN_RING_CLOBBER                                                                                                             \
  "v192", "v193", "v194", "v195", "v196", "v197", "v198", "v199", "v200", "v201", "v202", "v203", "v204", "v205", "v206", "v207",   \
  "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", "v216", "v217", "v218", "v219", "v220", "v221", "v222", "v223",   \
  "v224", "v225", "v226", "v227", "v228", "v229", "v230", "v231", "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239",   \
  "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251", "v252", "v253", "v254", "v255"
#define TN_RING_FENCE() asm volatile("" ::: TN_RING_CLOBBER)
constexpr int ring_reg(int rs, int kq, int f) { return TN_RING_BASE + ((rs * 4 + kq) * 2 + f) * 4; }   // [super-step parity][k-step][fragment] x 4 dwords

// ================= device side: statements both kernels issue between their MFMA slots =================
// Shared here are the statements that could be moved without changing a single instruction of either kernel's listing: the counted
// ring wait, the ring refill and the DMA statements of an interval.  The state they work on (dsrc / ddst / cdelta, voff[]) stays in
// the kernels and is passed in.  P is the kernel's policy type: kPlaneB (bytes of one k-step plane of the kernel's private
// k-step-major frame copy) and kExp (the 14x14 kernel's TN_B14_EXP timing-experiment bits; 0 in the 28x28 kernel).
// NOT shared (docs/kernels.md has the listing differences seen): advance_dma, begin_interval / end_interval, bn_ring / bn_dword,
// consts_read / wa_read / w3_read, epa_item(s), pre_item / kPreItems and the intervals themselves.

// a ring register pair is waited for two super-step intervals after its refills (kVmRing)
__device__ __forceinline__ void ring_wait() { asm volatile("s_waitcnt vmcnt(%c0)" ::"n"(kVmRing) : TN_RING_CLOBBER); }
// a ring refill: the lane's 16 B (voff[F]) of fragment F of k-step KQ of the planes at `base` into the literal registers of ring slot RS
template <typename P, int RS, int KQ, int F>
__device__ __forceinline__ void ring_load(ic<RS>, ic<KQ>, ic<F>, const unsigned char *base, const unsigned (&voff)[2], unsigned lane16, int wid) {
  constexpr int R = ring_reg(RS, KQ, F);
  if (P::kExp & 1) return;
  const unsigned vo = (P::kExp & 16) ? lane16 + (unsigned)(wid * 8 + F * 4 + KQ) * 1024u : voff[F];
  const unsigned char *pb = base + KQ * P::kPlaneB;
  asm volatile("global_load_dwordx4 v[%c0:%c1], %2, %3" ::"n"(R), "n"(R + 3), "v"(vo), "s"(pb) : TN_RING_CLOBBER);
}
// the DMA statements of an interval: this wave's part of unit g + 4 - two pairs of 1-KiB fragment pieces (PR = 0, 1) and its piece
// of the constants - from dsrc to the LDS address ddst; cdelta: from the fragment part to the constants piece
template <typename P, int PR>
__device__ __forceinline__ void stream_dma_pair(ic<PR>, const unsigned char *dsrc, unsigned lane16, unsigned ddst) {
  if (P::kExp & 8) return;
  dma16x2<PR * 2048>(dsrc, lane16, ddst);
}
template <typename P>
__device__ __forceinline__ void stream_dma_consts(const unsigned char *dsrc, int cdelta, unsigned lane4, unsigned ddst) {
  if (P::kExp & 8) return;
  dma4(dsrc + cdelta, lane4, ddst + cdelta);
}

// ================= host side: one unit of the stream =================
// Every unit is kUnitBytes = 16 fragments [64 lanes][8 halfs] + 128 floats' worth of BN1 constants.  A packer (pack_block14 /
// pack_block28) only decides the ORDER of units; what a unit of each kind holds is written here, next to the code that reads it.
struct StreamWriter {
  std::vector<unsigned char> &out;
  f16 *frag(size_t u, int fi) const { return (f16 *)(out.data() + u * kUnitBytes + (size_t)fi * 1024); }
  f16 *cons(size_t u, int q, int h) const { return (f16 *)(out.data() + u * kUnitBytes + kUnitFrag + (q * 2 + h) * 64); }
  // channel j (0 .. 7) of a (k-step, half) group: dword J = j >> 1 holds halves (a[2J], a[2J+1]) | (b[2J], b[2J+1]) | 8 B unused
  static void put_const(f16 *d, int j, float a, float b) {
    d[8 * (j >> 1) + (j & 1)] = (f16)a;
    d[8 * (j >> 1) + 2 + (j & 1)] = (f16)b;
  }
  // the shift k-step of dense_strip.hip (fp16 hi + lo of BN2's shift, and 1 for the mask) in fragments f0 .. f0 + 3 of unit u
  void put_shift(size_t u, int f0, const Block14Layer &L) const {
    for (int mb = 0; mb < 4; ++mb) {
      f16 *d = frag(u, f0 + mb);
      for (int ln = 0; ln < 32; ++ln) {
        const float t = L.t2[32 * mb + ln];
        d[ln * 8 + 0] = (f16)t;
        d[ln * 8 + 1] = (f16)(t - (float)d[ln * 8 + 0]);
        d[ln * 8 + 2] = (f16)1.f;
      }
    }
  }
  // super-step unit su of a layer with K input channels, channels [64 su, 64 su + 64) clipped at `limit`: fragment (q, mb): lane l,
  // j: bottleneck channel 32 mb + (l & 31), input channel c = 64 su + 16 q + 8 (l >> 5) + j (zero weight and zero constants for
  // c >= limit); constants (q, h), dword J: halves a1[c + 2 J], a1[c + 2 J + 1], b1[c + 2 J], b1[c + 2 J + 1] (+ 8 B unused) for
  // c = 64 su + 16 q + 8 h (s1 / t1 of Block14Layer are those fp16 numbers: bn_relu_fold_fp16)
  void put_superstep(size_t u, const Block14Layer &L, int K, int su, int limit) const {
    for (int q = 0; q < 4; ++q) {
      for (int mb = 0; mb < 4; ++mb) {
        f16 *d = frag(u, q * 4 + mb);
        for (int ln = 0; ln < 64; ++ln)
          for (int j = 0; j < 8; ++j) {
            const int c = 64 * su + 16 * q + 8 * (ln >> 5) + j;
            d[ln * 8 + j] = c < limit ? (f16)L.w1f[(size_t)(32 * mb + (ln & 31)) * K + c] : (f16)0.f;
          }
      }
      for (int h = 0; h < 2; ++h) {
        f16 *d = cons(u, q, h);
        for (int j = 0; j < 8; ++j) {
          const int c = 64 * su + 16 * q + 8 * h + j;
          put_const(d, j, c < limit ? L.s1[c] : 0.f, c < limit ? L.t1[c] : 0.f);
        }
      }
    }
  }
  // 3x3 unit J: fragments (step 4 J + s, dx) at s * 3 + dx, s = 0 .. 3: kernel row ky_order[step / 8], tuple t = step % 8; lane
  // layout as pack_w3_strip (dense_strip.hip)
  void put_3x3(size_t u, const Block14Layer &L, int J, const std::array<int, 3> &ky_order) const {
    for (int s = 0; s < 4; ++s) {
      const int step = 4 * J + s, ky = ky_order[step / 8], t = step % 8;
      for (int dx = 0; dx < 3; ++dx) {
        f16 *d = frag(u, s * 3 + dx);
        for (int ln = 0; ln < 64; ++ln)
          for (int j = 0; j < 8; ++j) {
            const int m = ln & 31, o = 16 * ((m >> 2) & 1) + (m & 3) + 4 * (m >> 3);
            const int c = 16 * t + 8 * (j >> 2) + 4 * (ln >> 5) + (j & 3);
            d[ln * 8 + j] = (f16)L.w3[(((size_t)o * 128 + c) * 3 + ky) * 3 + dx];
          }
      }
    }
  }
};

// One launch helper for both kernels: the operand checks, the once-per-device opt-in to the kernel's dynamic LDS, the launch.
// `supported` / `units`: the kernel's own dense_blockNN_supported / dense_blockNN_units for (a.K0, a.nl); hw, range: the map size and
// the accepted range in words - every refusal names the geometry it was asked for.
template <void (*KERNEL)(DenseStreamArgs)>
int launch_stream_block(const char *name, int hw, const char *range, const DenseStreamArgs &a, bool supported, int units, int lds_bytes, hipStream_t s) {
  TN_REQUIRE(a.buf && a.stream && a.scratch, std::string(name) + ": null operand");
  const std::string geom = std::to_string(hw) + " x " + std::to_string(hw) + ", K0 = " + std::to_string(a.K0) + ", nl = " + std::to_string(a.nl) +
                           ", ldc = " + std::to_string(a.ldc) + ", B = " + std::to_string(a.B);
  TN_REQUIRE(supported, std::string(name) + ": unsupported geometry (this kernel runs " + range + "): " + geom);
  TN_REQUIRE(a.ldc % 64 == 0, std::string(name) + ": the row pitch must be a multiple of 64: " + geom);
  TN_REQUIRE(a.K0 + 32 * a.nl <= a.ldc, std::string(name) + ": the row pitch does not hold the last layer's output: " + geom);
  TN_REQUIRE(a.B > 0, std::string(name) + ": the batch must be positive: " + geom);
  TN_REQUIRE(a.total_units == units, std::string(name) + ": stream does not match the block");
  TN_SET_ATTR_ONCE_PER_DEVICE(TN_HIP_CHECK(hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes)));
  hipLaunchKernelGGL(KERNEL, dim3(a.B), dim3(256), lds_bytes, s, a);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

}  // namespace
