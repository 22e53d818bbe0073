// The fp32 encoder mode (TN_ENC_FP32, include/tennis_hip.h): every activation is stored in fp32 and every product is formed
// in fp32, on the f32-input MFMA v_mfma_f32_32x32x2_f32 (bit for bit a k-ordered fmaf chain; gfx950 has no xf32).  The weights
// are the raw fp32 parameters: no fp16 conversion, no hi + lo split, no clamp form, no centring.
//
// One implicit-GEMM kernel serves every convolution: rows are output pixels (M = B Ho Wo), columns output channels, and the
// operand loader of each kind builds the A tile from the fp32 activation map as it stages it into LDS:
//   FP32_STEM   7x7 stride-2 pad-3 conv of the input frames, normalised on load (uint8: the fp32 formula of
//               weights.normalize_to_nchw_f32, so a uint8 batch and its host-normalised copy are the same operand), k = c 49 + ky 7 + kx;
//               epilogue BatchNorm + ReLU
//   FP32_1X1    a dense layer's 1x1: BN1 + ReLU on load of the concat buffer's first K channels -> the raw bottleneck
//   FP32_3X3    a dense layer's 3x3, pad 1: BN2 + ReLU on load of the bottleneck, k = tap 128 + c, zero padding AFTER the
//               activation -> channels [yoff, yoff + 32) of the concat buffer
//   FP32_TRANS  a transition: BN + ReLU, then the 2x2 average (before the GEMM: the conv is linear), then the 1x1
// The workgroup (4 waves) computes a (128 TM) x (32 TN) tile, each wave TM x TN 32x32 MFMA tiles over its 32 TM rows (smaller
// tiles for small maps: launch_conv_fp32).  The k loop stages 32 k at a time: A as [row][33] (the operand reads one column of 32
// rows: conflict-free), B as [k][BN], the next stage's global loads in flight while the current one is multiplied.
#include <cmath>

#include "common.h"

namespace {

constexpr int kBK = 32;            // k per LDS stage
constexpr int kLdA = kBK + 1;      // row pitch of the A tile in floats
constexpr float kMeanF[3] = {0.485f, 0.456f, 0.406f}, kStdF[3] = {0.229f, 0.224f, 0.225f};   // weights.IMAGENET_MEAN / _STD (float32)

__device__ __forceinline__ float relu_bn(float v, float s, float t) { return fmaxf(fmaf(v, s, t), 0.f); }
__device__ __forceinline__ float4 relu_bn4(float4 v, float4 s, float4 t) {
  return make_float4(relu_bn(v.x, s.x, t.x), relu_bn(v.y, s.y, t.y), relu_bn(v.z, s.z, t.z), relu_bn(v.w, s.w, t.w));
}

// one normalised input value of frame b, channel c, pixel (iy, ix) (inside the frame)
__device__ __forceinline__ float stem_input(const void *x, int layout, long b, int c, int iy, int ix, int H, int W) {
  if (layout == TN_LAYOUT_NHWC_U8) {
    const float u = (float)((const unsigned char *)x)[((b * H + iy) * W + ix) * 3 + c];
    return __fdiv_rn(__fsub_rn(__fdiv_rn(u, 255.0f), kMeanF[c]), kStdF[c]);   // (x / 255 - mean) / std, each step rounded once
  }
  if (layout == TN_LAYOUT_NCHW_F32) return ((const float *)x)[((b * 3 + c) * H + iy) * W + ix];
  return (float)((const f16 *)x)[((b * H + iy) * W + ix) * 3 + c];
}

template <int KIND, int TM, int TN>
__global__ __launch_bounds__(256) void conv_fp32_kernel(const Fp32ConvArgs a) {
  constexpr int BM = 128 * TM, BN = 32 * TN;
  constexpr int AV = BM * kBK / 4 / 256;   // float4 of the A tile per thread
  constexpr int BV = kBK * BN / 4 / 256;   // float4 of the B tile per thread
  __shared__ float As[BM * kLdA];
  __shared__ __attribute__((aligned(16))) float Bs[kBK * BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long m0 = (long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int Kp = (a.K + kBK - 1) / kBK * kBK;

  // A slot i of this thread: tile row (tid >> 3) + 32 i, k quad tid & 7 of the stage
  long pb[AV];
  int py[AV], px[AV];
  bool pv[AV];
#pragma unroll
  for (int i = 0; i < AV; ++i) {
    const long m = m0 + (tid >> 3) + 32 * i;
    pv[i] = m < a.M;
    const long mm = pv[i] ? m : 0;
    px[i] = (int)(mm % a.Wo);
    py[i] = (int)((mm / a.Wo) % a.Ho);
    pb[i] = mm / ((long)a.Wo * a.Ho);
  }
  const int kq = (tid & 7) * 4;

  auto load_a = [&](int i, int k0) -> float4 {
    const int k = k0 + kq;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!pv[i]) return r;
    if constexpr (KIND == FP32_1X1) {
      const float *p = (const float *)a.x + ((pb[i] * a.H + py[i]) * a.W + px[i]) * a.ldx + k;
      r = relu_bn4(*(const float4 *)p, *(const float4 *)(a.s + k), *(const float4 *)(a.t + k));
    } else if constexpr (KIND == FP32_3X3) {
      const int tap = k >> 7, c = k & 127;
      const int iy = py[i] + tap / 3 - 1, ix = px[i] + tap % 3 - 1;
      if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
        const float *p = (const float *)a.x + ((pb[i] * a.H + iy) * a.W + ix) * a.ldx + c;
        r = relu_bn4(*(const float4 *)p, *(const float4 *)(a.s + c), *(const float4 *)(a.t + c));
      }
    } else if constexpr (KIND == FP32_TRANS) {
      const float4 s = *(const float4 *)(a.s + k), t = *(const float4 *)(a.t + k);
      const float *p = (const float *)a.x + ((pb[i] * a.H + 2 * py[i]) * a.W + 2 * px[i]) * a.ldx + k;
      const long row = (long)a.W * a.ldx;
      const float4 v00 = relu_bn4(*(const float4 *)p, s, t), v01 = relu_bn4(*(const float4 *)(p + a.ldx), s, t);
      const float4 v10 = relu_bn4(*(const float4 *)(p + row), s, t), v11 = relu_bn4(*(const float4 *)(p + row + a.ldx), s, t);
      r = make_float4(((v00.x + v01.x) + (v10.x + v11.x)) * 0.25f, ((v00.y + v01.y) + (v10.y + v11.y)) * 0.25f,
                      ((v00.z + v01.z) + (v10.z + v11.z)) * 0.25f, ((v00.w + v01.w) + (v10.w + v11.w)) * 0.25f);
    } else {   // FP32_STEM
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = 0.f;
        const int kk = k + j;
        if (kk < a.K) {
          const int c = kk / 49, r49 = kk % 49;
          const int iy = 2 * py[i] - 3 + r49 / 7, ix = 2 * px[i] - 3 + r49 % 7;
          if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v[j] = stem_input(a.x, a.layout, pb[i], c, iy, ix, a.H, a.W);
        }
      }
      r = make_float4(v[0], v[1], v[2], v[3]);
    }
    return r;
  };
  auto load_b = [&](int i, int k0) -> float4 {
    const int f = tid + 256 * i, kr = f / (BN / 4), c4 = f % (BN / 4);
    return *(const float4 *)(a.w + (long)(k0 + kr) * a.N + n0 + 4 * c4);
  };

  float4 ra[AV], rb[BV];
#pragma unroll
  for (int i = 0; i < AV; ++i) ra[i] = load_a(i, 0);
#pragma unroll
  for (int i = 0; i < BV; ++i) rb[i] = load_b(i, 0);

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
    for (int i = 0; i < AV; ++i) {
      float *q = As + ((tid >> 3) + 32 * i) * kLdA + kq;
      q[0] = ra[i].x; q[1] = ra[i].y; q[2] = ra[i].z; q[3] = ra[i].w;
    }
#pragma unroll
    for (int i = 0; i < BV; ++i) {
      const int f = tid + 256 * i;
      *(float4 *)(Bs + (f / (BN / 4)) * BN + 4 * (f % (BN / 4))) = rb[i];
    }
    __syncthreads();
    if (k0 + kBK < Kp) {
#pragma unroll
      for (int i = 0; i < AV; ++i) ra[i] = load_a(i, k0 + kBK);
#pragma unroll
      for (int i = 0; i < BV; ++i) rb[i] = load_b(i, k0 + kBK);
    }
    // 32x32x2: lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]
#pragma unroll
    for (int kk = 0; kk < kBK / 2; ++kk) {
      const int kr = 2 * kk + (lane >> 5);
      float av[TM], bv[TN];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) av[tm] = As[(wave * 32 * TM + tm * 32 + (lane & 31)) * kLdA + kr];
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) bv[tn] = Bs[kr * BN + tn * 32 + (lane & 31)];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm], bv[tn], acc[tm][tn], 0, 0, 0);
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

__global__ void maxpool_fp32_kernel(const float *__restrict__ x, int B, int H, int W, float *__restrict__ y, int ldy, int Ho, int Wo) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // (b, oy, ox, channel quad)
  if (i >= (long)B * Ho * Wo * 16) return;
  const int c = (int)(i & 15) * 4;
  long p = i >> 4;
  const int ox = (int)(p % Wo);
  p /= Wo;
  const int oy = (int)(p % Ho);
  const long b = p / Ho;
  float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int iy = 2 * oy + dy, ix = 2 * ox + dx;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      const float4 v = *(const float4 *)(x + ((b * H + iy) * W + ix) * 64 + c);
      m = make_float4(fmaxf(m.x, v.x), fmaxf(m.y, v.y), fmaxf(m.z, v.z), fmaxf(m.w, v.w));
    }
  *(float4 *)(y + ((b * Ho + oy) * Wo + ox) * ldy + c) = m;
}

template <int KIND, int TM, int TN>
int launch_kind(const Fp32ConvArgs &a, hipStream_t s) {
  TN_REQUIRE(a.N % (32 * TN) == 0, "conv_fp32: output channels must be a multiple of the tile width");
  const long blocks = ((long)a.M + 128 * TM - 1) / (128 * TM);
  hipLaunchKernelGGL((conv_fp32_kernel<KIND, TM, TN>), dim3((unsigned)blocks, a.N / (32 * TN)), dim3(256), 0, s, a);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

}  // namespace

int launch_conv_fp32(const Fp32ConvArgs &a, hipStream_t s, int tile) {
  TN_REQUIRE(a.M > 0 && a.K > 0 && a.x && a.w && a.y, "conv_fp32: empty or null operand");
  TN_REQUIRE(tile >= 0 && tile <= 2, "conv_fp32: tile selector must be 0 (the launcher's choice), 1 (small) or 2 (large)");
  // The k loop runs to K rounded up to the k-stage and reads s, t, the activation's channels and the weight rows that far: only the
  // stem's loader stops at K (its weight array carries the zero rows), every other kind needs K to be a whole number of stages.
  TN_REQUIRE(a.kind == FP32_STEM || (a.ldx % 4 == 0 && a.K % kBK == 0 && a.s && a.t),
             "conv_fp32: channel strides must be multiples of 4 and K a multiple of the k-stage (32)");
  TN_REQUIRE(a.kind == FP32_STEM || (((uintptr_t)a.x | (uintptr_t)a.s | (uintptr_t)a.t) & 15) == 0, "conv_fp32: operands must be 16-byte aligned");
  TN_REQUIRE(((uintptr_t)a.w & 15) == 0, "conv_fp32: the weight array must be 16-byte aligned");
  TN_REQUIRE(a.N % 32 == 0 && a.ldy % 4 == 0 && a.yoff % 4 == 0 && a.yoff + a.N <= a.ldy, "conv_fp32: output columns out of range");
  // Where the large tile leaves fewer than two workgroups per CU (the 28 x 28 and smaller maps of a 224 x 224 input), half the tile:
  // every output value is the same k-ordered chain whatever the tile, so the choice changes no bit of the result.
  auto tiles = [&](int bm, int bn) { return ((long)a.M + bm - 1) / bm * (a.N / bn); };
  const bool big = tile ? tile == 2 : tiles(128, 128) >= 512;
  switch (a.kind) {
    case FP32_STEM: return launch_kind<FP32_STEM, 1, 2>(a, s);
    case FP32_1X1:
      TN_REQUIRE(a.ldx >= a.K, "conv_fp32: K beyond the channel stride");
      return big ? launch_kind<FP32_1X1, 1, 4>(a, s) : launch_kind<FP32_1X1, 1, 2>(a, s);
    case FP32_3X3:
      TN_REQUIRE(a.K == 9 * 128 && a.ldx == 128, "conv_fp32: the 3x3 reads a dense 128-channel bottleneck");
      return (tile ? tile == 2 : tiles(256, 32) >= 512) ? launch_kind<FP32_3X3, 2, 1>(a, s) : launch_kind<FP32_3X3, 1, 1>(a, s);
    case FP32_TRANS:
      TN_REQUIRE(a.ldx >= a.K, "conv_fp32: K beyond the channel stride");
      TN_REQUIRE(2 * a.Ho <= a.H && 2 * a.Wo <= a.W, "conv_fp32: transition output larger than half its input");
      return big ? launch_kind<FP32_TRANS, 1, 4>(a, s) : launch_kind<FP32_TRANS, 1, 2>(a, s);
  }
  TN_REQUIRE(false, "conv_fp32: unknown kind");
}

int launch_maxpool_fp32(const float *x, int B, int H, int W, float *y, int ldy, int Ho, int Wo, hipStream_t s) {
  TN_REQUIRE(ldy % 4 == 0 && ldy >= 64, "maxpool_fp32: bad output stride");
  const long total = (long)B * Ho * Wo * 16;
  hipLaunchKernelGGL(maxpool_fp32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, B, H, W, y, ldy, Ho, Wo);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}
