// Class activation maps of the frame classifier (tn_densenet121_forward_class_maps).  The network ends in
// BN -> ReLU -> AvgPool2D(7) -> Flatten -> Dense, so a logit is a plain sum over the cells of the last feature map:
//   A[b,k,y,x]   = relu(scale[k] * map[b,y,x,k] + shift[k])                                  (what head_kernel averages, pool.hip)
//   cam[b,c,y,x] = (1/49) * sum_k Wd[c, k*PH*PW + (y/7)*PW + (x/7)] * A[b,k,y,x]              0 <= y < 7 PH, 0 <= x < 7 PW
//   logit[b,c]   = bias[c] + sum_{y,x} cam[b,c,y,x]
// One WAVE owns PIX consecutive cells (ky*7 + kx order) of one 7x7 pool window of one frame; lane l owns the 8-channel chunks
// l, l + 64, ... of those cells (16 bytes per lane and load, as head_kernel reads them; every map value is read once).  The
// Dense weights of a chunk are loaded once per class and used for all PIX cells.  A lane accumulates its chunks in ascending
// order, 8 channels each in ascending order; the 64 lanes are then summed by a six-level xor tree (32, 16, 8, 4, 2, 1) run as
// a reduce-scatter, so that every lane ends up with two finished values and stores them.  No atomics, and nothing of that
// order depends on the batch size, the frame's position in the batch or the grid: results are bit-reproducible.
//   kClassMapsSeq(C) = 8 * ceil(C / 512) sequential fp32 fmas per lane, kClassMapsDepth = 6 butterfly levels.
#include "common.h"

namespace {

constexpr int kClassMapsDepth = 6;

// NC: class slots per lane (classes <= NC), PIX: cells per wave
template <bool X32, int NC, int PIX>
__global__ __launch_bounds__(256) void class_maps_kernel(const f16 *__restrict__ x, const float *__restrict__ x32, int B, int H, int W, int C,
                                                         const float *__restrict__ scale, const float *__restrict__ shift,
                                                         const float *__restrict__ wd, int PH, int PW, int classes, float *__restrict__ out) {
  constexpr int NG = (49 + PIX - 1) / PIX;      // cell groups per pool window
  const int lane = threadIdx.x & 63;
  const long total = (long)B * PH * PW * NG;
  const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= total) return;                     // (whole waves; the kernel has no barrier)
  const int grp = (int)(wid % NG);
  long q = wid / NG;
  const int pw = (int)(q % PW);
  q /= PW;
  const int ph = (int)(q % PH);
  const int b = (int)(q / PH);
  const int PP = PH * PW, cell = ph * PW + pw;
  const long F = (long)C * PP;
  const int cpp = C >> 3;
  float acc[PIX][NC];
#pragma unroll
  for (int p = 0; p < PIX; ++p)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[p][c] = 0.f;
  for (int ch = lane; ch < cpp; ch += 64) {
    float sc[8], sh[8], a[PIX][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sc[j] = scale[ch * 8 + j];
      sh[j] = shift[ch * 8 + j];
    }
#pragma unroll
    for (int p = 0; p < PIX; ++p) {
      const int pi = grp * PIX + p;
      if (pi < 49) {
        const int iy = ph * 7 + pi / 7, ix = pw * 7 + pi % 7;
        const long off = (((long)b * H + iy) * W + ix) * C + ch * 8;
        if constexpr (X32) {
          const float4 *s4 = (const float4 *)(x32 + off);
          const float4 v0 = s4[0], v1 = s4[1];
          const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
          for (int j = 0; j < 8; ++j) a[p][j] = fmaxf(fmaf(v[j], sc[j], sh[j]), 0.f);
        } else {
          const f16x8 v = *(const f16x8 *)(x + off);
#pragma unroll
          for (int j = 0; j < 8; ++j) a[p][j] = fmaxf(fmaf((float)v[j], sc[j], sh[j]), 0.f);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) a[p][j] = 0.f;
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c < classes) {
        const float *wr = wd + (long)c * F + (long)ch * 8 * PP + cell;      // channel k of this window: wr[(k - 8 ch) * PP]
        float w[8];
        if (PP == 1) {
          const float4 w0 = ((const float4 *)wr)[0], w1 = ((const float4 *)wr)[1];
          w[0] = w0.x; w[1] = w0.y; w[2] = w0.z; w[3] = w0.w; w[4] = w1.x; w[5] = w1.y; w[6] = w1.z; w[7] = w1.w;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) w[j] = wr[(long)j * PP];
        }
#pragma unroll
        for (int p = 0; p < PIX; ++p)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[p][c] = fmaf(w[j], a[p][j], acc[p][c]);
      }
    }
  }
  // The 64 lanes' partial sums of the PIX * NC values, as a reduce-scatter: at level s (xor mask 32 >> s) a lane keeps the half of
  // its values its bit 5 - s selects, adds the partner's partial sums of that half, and hands the other half over.  After the six
  // levels lane l holds the finished values 2 l and 2 l + 1 (index p * NC + c); every value went through the same six-level
  // tree over the lanes, whatever the batch or the grid.  126 cross-lane moves instead of 6 per value, and every lane stores.
  static_assert(PIX * NC <= 128, "the reduce-scatter leaves two values per lane");
  float v[128];
#pragma unroll
  for (int i = 0; i < 128; ++i) v[i] = i < PIX * NC ? acc[i / NC][i % NC] : 0.f;
#pragma unroll
  for (int s = 0; s < kClassMapsDepth; ++s) {
    const int half = 64 >> s;
    const bool up = (lane >> (5 - s)) & 1;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const float keep = up ? v[i + half] : v[i], give = up ? v[i] : v[i + half];
      v[i] = keep + __shfl_xor(give, 32 >> s, 64);
    }
  }
  const int OH = 7 * PH, OW = 7 * PW;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int idx = 2 * lane + i, p = idx / NC, c = idx % NC, pi = grp * PIX + p;
    if (p < PIX && c < classes && pi < 49)
      out[(((long)b * classes + c) * OH + (ph * 7 + pi / 7)) * OW + (pw * 7 + pi % 7)] = v[i] * (1.0f / 49.0f);
  }
}

template <bool X32, int NC, int PIX>
void launch_one(const f16 *x, const float *x32, int B, int H, int W, int C, const float *scale, const float *shift, const float *wd,
                int PH, int PW, int classes, float *out, hipStream_t s) {
  const long waves = (long)B * PH * PW * ((49 + PIX - 1) / PIX);
  hipLaunchKernelGGL((class_maps_kernel<X32, NC, PIX>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, x, x32, B, H, W, C, scale, shift,
                     wd, PH, PW, classes, out);
}

}  // namespace

int class_maps_seq(int C) { return 8 * ((C / 8 + 63) / 64); }
int class_maps_depth() { return kClassMapsDepth; }

// map: x (fp16) or - non-null - x32 (fp32), NHWC (B, H, W, C); wd (classes, C PH PW) fp32; out (B, classes, 7 PH, 7 PW) fp32
int launch_class_maps(const f16 *x, const float *x32, int B, int H, int W, int C, const float *scale, const float *shift, const float *wd,
                      int PH, int PW, int classes, float *out, hipStream_t s) {
  TN_REQUIRE(C > 0 && C % 8 == 0, "class_maps: channels must be a multiple of 8");
  TN_REQUIRE(classes >= 1 && classes <= 64, "class_maps: classes must be in [1, 64]");
  TN_REQUIRE(B > 0 && PH > 0 && PW > 0 && 7 * PH <= H && 7 * PW <= W, "class_maps: bad shape (PH x PW windows of 7 x 7 inside H x W)");
  TN_REQUIRE((long)B * PH * PW * 49 < (1l << 31), "class_maps: too many cells for one launch");
#define TN_CAM_LAUNCH(X32) \
  do { \
    if (classes <= 16) launch_one<X32, 16, 7>(x, x32, B, H, W, C, scale, shift, wd, PH, PW, classes, out, s); \
    else if (classes <= 32) launch_one<X32, 32, 3>(x, x32, B, H, W, C, scale, shift, wd, PH, PW, classes, out, s); \
    else launch_one<X32, 64, 2>(x, x32, B, H, W, C, scale, shift, wd, PH, PW, classes, out, s); \
  } while (0)
  if (x32) TN_CAM_LAUNCH(true);
  else TN_CAM_LAUNCH(false);
#undef TN_CAM_LAUNCH
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}
