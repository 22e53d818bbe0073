// The fp32x3 encoder mode (TN_ENC_FP32X3, include/tennis_hip.h): the fp32 mode's network - fp32 activation maps, fp32
// accumulators, the same operand formulas, epilogue, max pool and head (dense_fp32.hip) - with the products on the bf16 matrix
// pipe.  Every fp32 operand value v is handed over as three bf16 terms
//   v1 = bf16(v),  v2 = bf16(v - v1),  v3 = bf16(v - v1 - v2)        (round to nearest even; the fp32 subtractions are exact)
// which carry 24 bits of v between them, and bf16 has fp32's exponent range: no scaling, no calibration, any checkpoint.  Of the
// nine cross products the six largest are formed, per 16-wide k-step and in this order, into ONE fp32 accumulator set:
//   a1 b1, a1 b2, a2 b1, a2 b2, a1 b3, a3 b1                        (v_mfma_f32_32x32x16_bf16; dropped: a2 b3, a3 b2, a3 b3 <= 2^-24 |a||b|)
// The order is the same for every tile shape, so an output value is the same bits whichever variant launch_conv_fp32x3 picks.
// (A value beyond bf16's largest finite number, 3.39e38, rounds to infinity in v1 and the split is NaN: no activation is.)
//
// A operand: the loader of each kind computes the fp32 value exactly as conv_fp32_kernel does (input normalisation, relu_bn, zero
// padding after the activation, the 2x2 average before the GEMM), splits it in registers and writes three bf16 LDS planes
// [row][32 k], 64-byte rows whose four 16-byte chunks are XOR-ed with (row >> 2) & 3: the fragment read of the 32x32x16 operand
// map (lane l: row l & 31, k = 8 (l >> 5) + j, 16 bytes) puts the 16 rows of each ds_read_b128 lane group on 16 different slots
// of the 256-byte bank row, with no padding.
// B operand: split once on the host (fp32x3_pack_weights) and stored in fragment order, [k-stage][32 columns][term][k-step][lane]
// 16 bytes each: staging is straight 16-byte copies, the fragment read is lane-contiguous.
#include <cmath>
#include <cstring>

#include "common.h"

// ---- host: the three-term split and the B operand image ----
static inline uint16_t bf16_rne(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline float bf16_as_float(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float v;
  memcpy(&v, &u, 4);
  return v;
}

void fp32x3_split(const float *w, int64_t n, uint16_t *t1, uint16_t *t2, uint16_t *t3) {
  for (int64_t i = 0; i < n; ++i) {
    const uint16_t h1 = bf16_rne(w[i]);
    const float r1 = w[i] - bf16_as_float(h1);        // exact
    const uint16_t h2 = bf16_rne(r1);
    const float r2 = r1 - bf16_as_float(h2);          // exact
    t1[i] = h1; t2[i] = h2; t3[i] = bf16_rne(r2);
  }
}

// wk [kp][N] fp32 (k-major, zero rows past K, kp a multiple of 32, N of 32) -> the fragment image, 3 kp N bf16
std::vector<uint16_t> fp32x3_pack_weights(const float *wk, int kp, int N) {
  std::vector<uint16_t> t[3];
  for (auto &v : t) v.resize((size_t)kp * N);
  fp32x3_split(wk, (int64_t)kp * N, t[0].data(), t[1].data(), t[2].data());
  std::vector<uint16_t> o((size_t)3 * kp * N);
  size_t q = 0;
  for (int s = 0; s < kp / 32; ++s)
    for (int g = 0; g < N / 32; ++g)
      for (int p = 0; p < 3; ++p)
        for (int ks = 0; ks < 2; ++ks)
          for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j) o[q++] = t[p][(size_t)(s * 32 + ks * 16 + 8 * (l >> 5) + j) * N + g * 32 + (l & 31)];
  return o;
}

extern "C" int tn_fp32x3_split(const float *w, int64_t n, uint16_t *t1, uint16_t *t2, uint16_t *t3) {
  TN_REQUIRE(w && t1 && t2 && t3 && n >= 0, "tn_fp32x3_split: null argument");
  fp32x3_split(w, n, t1, t2, t3);
  return TN_OK;
}

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kBK = 32;            // k per LDS stage: two 16-wide k-steps
constexpr int kBFrag = 3 * 2 * 64; // 16-byte chunks of the B image per (k-stage, 32 columns)
constexpr float kMeanF[3] = {0.485f, 0.456f, 0.406f}, kStdF[3] = {0.229f, 0.224f, 0.225f};   // weights.IMAGENET_MEAN / _STD (float32)

__device__ __forceinline__ float relu_bn(float v, float s, float t) { return fmaxf(fmaf(v, s, t), 0.f); }
__device__ __forceinline__ float4 relu_bn4(float4 v, float4 s, float4 t) {
  return make_float4(relu_bn(v.x, s.x, t.x), relu_bn(v.y, s.y, t.y), relu_bn(v.z, s.z, t.z), relu_bn(v.w, s.w, t.w));
}

// one normalised input value of frame b, channel c, pixel (iy, ix) (inside the frame): dense_fp32.hip's formula
__device__ __forceinline__ float stem_input(const void *x, int layout, long b, int c, int iy, int ix, int H, int W) {
  if (layout == TN_LAYOUT_NHWC_U8) {
    const float u = (float)((const unsigned char *)x)[((b * H + iy) * W + ix) * 3 + c];
    return __fdiv_rn(__fsub_rn(__fdiv_rn(u, 255.0f), kMeanF[c]), kStdF[c]);   // (x / 255 - mean) / std, each step rounded once
  }
  if (layout == TN_LAYOUT_NCHW_F32) return ((const float *)x)[((b * 3 + c) * H + iy) * W + ix];
  return (float)((const f16 *)x)[((b * H + iy) * W + ix) * 3 + c];
}

// two fp32 values -> bf16 pair (round to nearest even), x in the low half
__device__ __forceinline__ unsigned cvt_pk_bf16(float x, float y) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
  return r;
}
// ... -> the three terms of both
__device__ __forceinline__ void split2(float x, float y, unsigned &p1, unsigned &p2, unsigned &p3) {
  p1 = cvt_pk_bf16(x, y);
  float rx = __fsub_rn(x, __uint_as_float(p1 << 16)), ry = __fsub_rn(y, __uint_as_float(p1 & 0xffff0000u));
  p2 = cvt_pk_bf16(rx, ry);
  rx = __fsub_rn(rx, __uint_as_float(p2 << 16));
  ry = __fsub_rn(ry, __uint_as_float(p2 & 0xffff0000u));
  p3 = cvt_pk_bf16(rx, ry);
}

struct F8 { float4 lo, hi; };

template <int KIND, int TM, int TN>
__global__ __launch_bounds__(256) void conv_fp32x3_kernel(const Fp32ConvArgs a) {
  constexpr int BM = 128 * TM, BN = 32 * TN;
  constexpr int NA = BM / 64;                  // 8-value slots of the A tile per thread
  constexpr int BCH = TN * kBFrag;             // 16-byte chunks of the B stage
  constexpr int NB = (BCH + 255) / 256;
  __shared__ uint4 As[3][BM * 4];              // [term][row][chunk ^ ((row >> 2) & 3)], a chunk = 8 k
  __shared__ uint4 Bs[BCH];                    // [32 columns][term][k-step][lane]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long m0 = (long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int Kp = (a.K + kBK - 1) / kBK * kBK;

  // A slot i of this thread: tile row (tid >> 2) + 64 i, k chunk tid & 3 of the stage
  long pb[NA];
  int py[NA], px[NA];
  bool pv[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const long m = m0 + (tid >> 2) + 64 * i;
    pv[i] = m < a.M;
    const long mm = pv[i] ? m : 0;
    px[i] = (int)(mm % a.Wo);
    py[i] = (int)((mm / a.Wo) % a.Ho);
    pb[i] = mm / ((long)a.Wo * a.Ho);
  }
  const int kc = (tid & 3) * 8;

  auto load_a = [&](int i, int k0) -> F8 {
    const int k = k0 + kc;
    F8 r{make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    if (!pv[i]) return r;
    if constexpr (KIND == FP32_1X1) {
      const float *p = (const float *)a.x + ((pb[i] * a.H + py[i]) * a.W + px[i]) * a.ldx + k;
      r.lo = relu_bn4(*(const float4 *)p, *(const float4 *)(a.s + k), *(const float4 *)(a.t + k));
      r.hi = relu_bn4(*(const float4 *)(p + 4), *(const float4 *)(a.s + k + 4), *(const float4 *)(a.t + k + 4));
    } else if constexpr (KIND == FP32_3X3) {
      const int tap = k >> 7, c = k & 127;
      const int iy = py[i] + tap / 3 - 1, ix = px[i] + tap % 3 - 1;
      if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
        const float *p = (const float *)a.x + ((pb[i] * a.H + iy) * a.W + ix) * a.ldx + c;
        r.lo = relu_bn4(*(const float4 *)p, *(const float4 *)(a.s + c), *(const float4 *)(a.t + c));
        r.hi = relu_bn4(*(const float4 *)(p + 4), *(const float4 *)(a.s + c + 4), *(const float4 *)(a.t + c + 4));
      }
    } else if constexpr (KIND == FP32_TRANS) {
      const float *p0 = (const float *)a.x + ((pb[i] * a.H + 2 * py[i]) * a.W + 2 * px[i]) * a.ldx + k;
      const long row = (long)a.W * a.ldx;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float4 s = *(const float4 *)(a.s + k + 4 * h), t = *(const float4 *)(a.t + k + 4 * h);
        const float *p = p0 + 4 * h;
        const float4 v00 = relu_bn4(*(const float4 *)p, s, t), v01 = relu_bn4(*(const float4 *)(p + a.ldx), s, t);
        const float4 v10 = relu_bn4(*(const float4 *)(p + row), s, t), v11 = relu_bn4(*(const float4 *)(p + row + a.ldx), s, t);
        (h ? r.hi : r.lo) = make_float4(((v00.x + v01.x) + (v10.x + v11.x)) * 0.25f, ((v00.y + v01.y) + (v10.y + v11.y)) * 0.25f,
                                        ((v00.z + v01.z) + (v10.z + v11.z)) * 0.25f, ((v00.w + v01.w) + (v10.w + v11.w)) * 0.25f);
      }
    } else {   // FP32_STEM
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[j] = 0.f;
        const int kk = k + j;
        if (kk < a.K) {
          const int c = kk / 49, r49 = kk % 49;
          const int iy = 2 * py[i] - 3 + r49 / 7, ix = 2 * px[i] - 3 + r49 % 7;
          if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v[j] = stem_input(a.x, a.layout, pb[i], c, iy, ix, a.H, a.W);
        }
      }
      r.lo = make_float4(v[0], v[1], v[2], v[3]);
      r.hi = make_float4(v[4], v[5], v[6], v[7]);
    }
    return r;
  };
  const uint4 *wimg = (const uint4 *)a.wx + (long)(n0 / 32) * kBFrag;
  const long wstage = (long)(a.N / 32) * kBFrag;      // chunks per k-stage of the whole image
  auto load_b = [&](int i, int k0) -> uint4 {
    const int f = tid + 256 * i;
    if (BCH % 256 != 0 && f >= BCH) return make_uint4(0u, 0u, 0u, 0u);
    return wimg[(long)(k0 / kBK) * wstage + f];
  };

  F8 ra[NA];
  uint4 rb[NB];
#pragma unroll
  for (int i = 0; i < NA; ++i) ra[i] = load_a(i, 0);
#pragma unroll
  for (int i = 0; i < NB; ++i) rb[i] = load_b(i, 0);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

  for (int k0 = 0; k0 < Kp; k0 += kBK) {
    __syncthreads();      // the previous stage has been read
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int row = (tid >> 2) + 64 * i;
      const int at = row * 4 + ((tid & 3) ^ ((row >> 2) & 3));
      uint4 p1, p2, p3;
      split2(ra[i].lo.x, ra[i].lo.y, p1.x, p2.x, p3.x);
      split2(ra[i].lo.z, ra[i].lo.w, p1.y, p2.y, p3.y);
      split2(ra[i].hi.x, ra[i].hi.y, p1.z, p2.z, p3.z);
      split2(ra[i].hi.z, ra[i].hi.w, p1.w, p2.w, p3.w);
      As[0][at] = p1; As[1][at] = p2; As[2][at] = p3;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int f = tid + 256 * i;
      if (BCH % 256 == 0 || f < BCH) Bs[f] = rb[i];
    }
    __syncthreads();
    if (k0 + kBK < Kp) {
#pragma unroll
      for (int i = 0; i < NA; ++i) ra[i] = load_a(i, k0 + kBK);
#pragma unroll
      for (int i = 0; i < NB; ++i) rb[i] = load_b(i, k0 + kBK);
    }
    // 32x32x16: lane l holds A[i = l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][j' = l & 31]
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[TM][3], bw[TN][3];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
        const int row = wave * 32 * TM + tm * 32 + (lane & 31);
        const int at = row * 4 + ((2 * ks + (lane >> 5)) ^ ((row >> 2) & 3));
#pragma unroll
        for (int p = 0; p < 3; ++p) af[tm][p] = __builtin_bit_cast(bf16x8, As[p][at]);
      }
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int p = 0; p < 3; ++p) bw[tn][p] = __builtin_bit_cast(bf16x8, Bs[tn * kBFrag + (p * 2 + ks) * 64 + lane]);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
          f32x16 c = acc[tm][tn];
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[tm][0], bw[tn][0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[tm][0], bw[tn][1], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[tm][1], bw[tn][0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[tm][1], bw[tn][1], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[tm][0], bw[tn][2], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[tm][2], bw[tn][0], c, 0, 0, 0);
          acc[tm][tn] = c;
        }
    }
  }

  // C/D: column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const int n = n0 + tn * 32 + (lane & 31);
      const float es = a.es ? a.es[n] : 1.f, et = a.es ? a.et[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long m = m0 + wave * 32 * TM + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= a.M) continue;
        const float v = a.es ? relu_bn(acc[tm][tn][r], es, et) : acc[tm][tn][r];
        a.y[m * a.ldy + a.yoff + n] = v;
      }
    }
}

template <int KIND, int TM, int TN>
int launch_kind(const Fp32ConvArgs &a, hipStream_t s) {
  TN_REQUIRE(a.N % (32 * TN) == 0, "conv_fp32x3: output channels must be a multiple of the tile width");
  const long blocks = ((long)a.M + 128 * TM - 1) / (128 * TM);
  hipLaunchKernelGGL((conv_fp32x3_kernel<KIND, TM, TN>), dim3((unsigned)blocks, a.N / (32 * TN)), dim3(256), 0, s, a);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

}  // namespace

int launch_conv_fp32x3(const Fp32ConvArgs &a, hipStream_t s, int tile) {
  TN_REQUIRE(a.M > 0 && a.K > 0 && a.x && a.wx && a.y, "conv_fp32x3: empty or null operand");
  TN_REQUIRE(tile >= 0 && tile <= 2, "conv_fp32x3: tile selector must be 0 (the launcher's choice), 1 (small) or 2 (large)");
  TN_REQUIRE(a.kind == FP32_STEM || (a.ldx % 4 == 0 && a.K % kBK == 0 && a.s && a.t),
             "conv_fp32x3: channel strides must be multiples of 4 and K a multiple of the k-stage (32)");
  TN_REQUIRE(a.kind == FP32_STEM || (((uintptr_t)a.x | (uintptr_t)a.s | (uintptr_t)a.t) & 15) == 0, "conv_fp32x3: operands must be 16-byte aligned");
  TN_REQUIRE(((uintptr_t)a.wx & 15) == 0, "conv_fp32x3: the weight image must be 16-byte aligned");
  TN_REQUIRE(a.N % 32 == 0 && a.ldy % 4 == 0 && a.yoff % 4 == 0 && a.yoff + a.N <= a.ldy, "conv_fp32x3: output columns out of range");
  // the tile shapes and the small-map halving of launch_conv_fp32; the fixed product order makes the choice invisible in the result
  auto tiles = [&](int bm, int bn) { return ((long)a.M + bm - 1) / bm * (a.N / bn); };
  const bool big = tile ? tile == 2 : tiles(128, 128) >= 512;
  switch (a.kind) {
    case FP32_STEM: return launch_kind<FP32_STEM, 1, 2>(a, s);
    case FP32_1X1:
      TN_REQUIRE(a.ldx >= a.K, "conv_fp32x3: K beyond the channel stride");
      return big ? launch_kind<FP32_1X1, 1, 4>(a, s) : launch_kind<FP32_1X1, 1, 2>(a, s);
    case FP32_3X3:
      TN_REQUIRE(a.K == 9 * 128 && a.ldx == 128, "conv_fp32x3: the 3x3 reads a dense 128-channel bottleneck");
      return (tile ? tile == 2 : tiles(256, 32) >= 512) ? launch_kind<FP32_3X3, 2, 1>(a, s) : launch_kind<FP32_3X3, 1, 1>(a, s);
    case FP32_TRANS:
      TN_REQUIRE(a.ldx >= a.K, "conv_fp32x3: K beyond the channel stride");
      TN_REQUIRE(2 * a.Ho <= a.H && 2 * a.Wo <= a.W, "conv_fp32x3: transition output larger than half its input");
      return big ? launch_kind<FP32_TRANS, 1, 4>(a, s) : launch_kind<FP32_TRANS, 1, 2>(a, s);
  }
  TN_REQUIRE(false, "conv_fp32x3: unknown kind");
}
