// Fine-tuning step of the frame classifier (second half): FrameModel(DenseNet-121 .features, Dense(classes))
// trained end to end the way reference train.py drives it when the backbone is not frozen (model 0006 of
// models/README.md): BatchNorm in training mode (batch statistics, running statistics updated), SoftmaxCrossEntropyLoss
// per sample (:324), backward of the summed losses (:419-421), gluon.Trainer 'sgd' .step(batch_size) with momentum and
// weight decay (:298-299,424).  fp32 throughout, as MXNet trains by default.
//
// This is the CORRECT-FIRST version: every convolution is a GEMM on the exact-f32 matrix pipe (linear.hip / train.hip's
// transposed GEMM) over NHWC activations — 1x1 convolutions directly on the dense block's concat buffer, 3x3 and the 7x7
// stem through an explicit im2col buffer — with small element-wise / reduction kernels for BatchNorm, ReLU and the pools.
// The dense connectivity is what the inference path uses: one (B*H*W, C_total) buffer per block, a layer reads channels
// [0,K) and writes [K,K+32); the gradient buffer of a block has the same shape and every layer ACCUMULATES into [0,K).
// Activations that backward needs and that are cheap to rebuild (BN+ReLU outputs, im2col) are recomputed, the bottleneck
// convolution outputs and the batch statistics are kept.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "api_internal.h"
#include "gemm_fp32x3.h"
#include "linear.h"
#include "train.h"

namespace {

constexpr float kEps = 1e-5f;        // gluon nn.BatchNorm(epsilon=1e-5)
constexpr float kBnMom = 0.9f;       // gluon nn.BatchNorm(momentum=0.9)

// ---- im2col ---------------------------------------------------------------------------------------------------------
// 7x7 stride 2 pad 3 on (B,H,W,3) -> (B*Ho*Wo, 147), column order (ky, kx, c)
__global__ void ft_im2col7_kernel(const float *__restrict__ x, int B, int H, int W, float *__restrict__ col) {
  const int Ho = H / 2, Wo = W / 2;
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)B * Ho * Wo * 49) return;
  const int tap = (int)(id % 49);
  const long m = id / 49;
  const int ox = (int)(m % Wo), oy = (int)((m / Wo) % Ho), b = (int)(m / ((long)Wo * Ho));
  const int ky = tap / 7, kx = tap - ky * 7;
  const int iy = oy * 2 - 3 + ky, ix = ox * 2 - 3 + kx;
  float v0 = 0.f, v1 = 0.f, v2 = 0.f;
  if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
    const float *p = x + (((long)b * H + iy) * W + ix) * 3;
    v0 = p[0]; v1 = p[1]; v2 = p[2];
  }
  float *o = col + m * 147 + tap * 3;
  o[0] = v0; o[1] = v1; o[2] = v2;
}
// 3x3 pad 1 on (B,H,W,C) contiguous -> (B*H*W, 9*C), column order (ky, kx, c)
// sc / sh non-null: the source is a pre-activation, relu(a * sc[c] + sh[c]) is applied on the way (padding stays zero)
__global__ void ft_im2col3_kernel(const float *__restrict__ a, int B, int H, int W, int C, float *__restrict__ col,
                                  const float *__restrict__ sc = nullptr, const float *__restrict__ sh = nullptr) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int C4 = C / 4;
  if (id >= (long)B * H * W * 9 * C4) return;
  const int c4 = (int)(id % C4);
  const int tap = (int)((id / C4) % 9);
  const long m = id / ((long)C4 * 9);
  const int x = (int)(m % W), y = (int)((m / W) % H), b = (int)(m / ((long)W * H));
  const int iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
    v = *(const float4 *)(a + (((long)b * H + iy) * W + ix) * C + c4 * 4);
    if (sc) {
      const float4 s4 = *(const float4 *)(sc + c4 * 4), h4 = *(const float4 *)(sh + c4 * 4);
      v.x = fmaxf(fmaf(v.x, s4.x, h4.x), 0.f); v.y = fmaxf(fmaf(v.y, s4.y, h4.y), 0.f);
      v.z = fmaxf(fmaf(v.z, s4.z, h4.z), 0.f); v.w = fmaxf(fmaf(v.w, s4.w, h4.w), 0.f);
    }
  }
  *(float4 *)(col + m * 9 * C + tap * C + c4 * 4) = v;
}
// transpose of im2col3 (gather form, deterministic): da[m][c] = sum over taps of dcol[neighbour(m, tap)][tap][c]
__global__ void ft_col2im3_kernel(const float *__restrict__ dcol, int B, int H, int W, int C, float *__restrict__ da) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int C4 = C / 4;
  if (id >= (long)B * H * W * C4) return;
  const int c4 = (int)(id % C4);
  const long m = id / C4;
  const int x = (int)(m % W), y = (int)((m / W) % H), b = (int)(m / ((long)W * H));
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    // output pixel (oy, ox) read this pixel through tap (ky, kx) iff oy + ky - 1 == y, ox + kx - 1 == x
    const int oy = y - (tap / 3 - 1), ox = x - (tap % 3 - 1);
    if (oy >= 0 && oy < H && ox >= 0 && ox < W) {
      const float4 v = *(const float4 *)(dcol + ((((long)b * H + oy) * W + ox) * 9 + tap) * C + c4 * 4);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  }
  *(float4 *)(da + m * C + c4 * 4) = acc;
}

// ---- BatchNorm (training mode) + ReLU ---------------------------------------------------------------------------------
// batch mean and biased variance of columns [0,C) of x (row stride ld).  Grid (C/64, RS): 64 columns x one of RS row slices
// per workgroup; one pass over the data as sums of (x - k) and (x - k)^2 about a shift k near the mean, slices added in order
// (in double) by the finish kernel, which forms var = s2/M - d^2 with d = s1/M.  That difference cancels (k - mean)^2 / var of
// its digits: k is the float64 mean of kStatSamples rows spread over the column, the same in every workgroup, so d is
// about sigma / 8 for any column.  (The column's first row, the shift this used to take, is a zero-padded convolution's corner
// pixel: 30 sigma from the mean it cost the variance three digits.)  A constant column gets k = the constant and var = 0 exactly.
constexpr int kStatSamples = 64;
__global__ __launch_bounds__(1024) void ft_bn_stats_kernel(const float *__restrict__ x, int ld, long M, int C,
                                                           float *__restrict__ part) {
  __shared__ float p1[16][64], p2[16][64];
  __shared__ double ks[16][64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
  const long stride = 16L * gridDim.y;
  // the shift: row group rg takes samples rg * 4 .. rg * 4 + 3, added in a fixed order.  Sample i is row frac((i + 1/2) phi) M:
  // spread over the column without a stride that a power-of-two frame could alias (an even stride puts every sample on a border)
  double k4 = 0.0;
  if (c < C) {
#pragma unroll
    for (int j = 0; j < kStatSamples / 16; ++j) {
      double f = (rg * (kStatSamples / 16) + j + 0.5) * 0.6180339887498949;
      f -= floor(f);
      const long r = min((long)(f * (double)M), M - 1);
      k4 += (double)x[r * ld + c];
    }
  }
  ks[rg][cl] = k4;
  __syncthreads();
  double ksum = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) ksum += ks[i][cl];
  const float k = (float)(ksum / kStatSamples);
  float a1 = 0.f, a2 = 0.f;
  if (c < C) {
    long r = (long)blockIdx.y * 16 + rg;
    for (; r + 15 * stride < M; r += 16 * stride) {
      float v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = x[(r + i * stride) * ld + c] - k;
#pragma unroll
      for (int i = 0; i < 16; ++i) { a1 += v[i]; a2 = fmaf(v[i], v[i], a2); }
    }
    for (; r < M; r += stride) { const float d = x[r * ld + c] - k; a1 += d; a2 = fmaf(d, d, a2); }
  }
  p1[rg][cl] = a1; p2[rg][cl] = a2;
  __syncthreads();
  if (rg == 0 && c < C) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { s1 += p1[i][cl]; s2 += p2[i][cl]; }
    part[((long)blockIdx.y * 2 + 0) * C + c] = s1;
    part[((long)blockIdx.y * 2 + 1) * C + c] = s2;
    if (blockIdx.y == 0) part[(long)gridDim.y * 2 * C + c] = k;
  }
}
__global__ void ft_bn_stats_finish_kernel(const float *__restrict__ part, int RS, int C, long M, float *__restrict__ mean,
                                          float *__restrict__ var) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
  for (int z = 0; z < RS; ++z) { s1 += part[((long)z * 2 + 0) * C + c]; s2 += part[((long)z * 2 + 1) * C + c]; }
  const double d = s1 / (double)M;
  mean[c] = (float)((double)part[(long)RS * 2 * C + c] + d);
  var[c] = (float)fmax(s2 / (double)M - d * d, 0.0);
}
// y (M,C contiguous) = relu(gamma * (x - mean) / sqrt(var + eps) + beta)
__global__ void ft_bn_relu_kernel(const float *__restrict__ x, int ld, long M, int C, const float *__restrict__ mean,
                                  const float *__restrict__ var, const float *__restrict__ gamma,
                                  const float *__restrict__ beta, float *__restrict__ y) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= M * C) return;
  const long r = id / C;
  const int c = (int)(id - r * C);
  const float v = gamma[c] * (x[r * ld + c] - mean[c]) * rsqrtf(var[c] + kEps) + beta[c];
  y[id] = v > 0.f ? v : 0.f;
}
// column sums the BN backward needs: s1 = sum g, s2 = sum g * xhat with g = dy * [bn output > 0].  Grid (C/64, RS): 64
// columns x one of RS row slices per workgroup (16 row groups inside), partial sums to part[(slice*2 + {0,1})*C + c];
// ft_bn_bwd_finish_kernel adds the slices in order.
__global__ __launch_bounds__(1024) void ft_bn_bwd_reduce_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                                int ld, long M, int C, const float *__restrict__ mean,
                                                                const float *__restrict__ var,
                                                                const float *__restrict__ gamma,
                                                                const float *__restrict__ beta, float *__restrict__ part) {
  __shared__ float p1[16][64], p2[16][64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
  const long stride = 16L * gridDim.y;
  float a1 = 0.f, a2 = 0.f;
  if (c < C) {
    const float m = mean[c], is = rsqrtf(var[c] + kEps), ga = gamma[c], be = beta[c];
    long r = (long)blockIdx.y * 16 + rg;
    for (; r + 7 * stride < M; r += 8 * stride) {
      float xv[8], dv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) { xv[i] = x[(r + i * stride) * ld + c]; dv[i] = dy[(r + i * stride) * C + c]; }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float xh = (xv[i] - m) * is;
        const float g = ga * xh + be > 0.f ? dv[i] : 0.f;
        a1 += g;
        a2 = fmaf(g, xh, a2);
      }
    }
    for (; r < M; r += stride) {
      const float xh = (x[r * ld + c] - m) * is;
      const float g = ga * xh + be > 0.f ? dy[r * C + c] : 0.f;
      a1 += g;
      a2 = fmaf(g, xh, a2);
    }
  }
  p1[rg][cl] = a1; p2[rg][cl] = a2;
  __syncthreads();
  if (rg == 0 && c < C) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { s1 += p1[i][cl]; s2 += p2[i][cl]; }
    part[((long)blockIdx.y * 2 + 0) * C + c] = s1;
    part[((long)blockIdx.y * 2 + 1) * C + c] = s2;
  }
}
__global__ void ft_bn_bwd_finish_kernel(const float *__restrict__ part, int RS, int C, float *__restrict__ dgamma,
                                        float *__restrict__ dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s1 = 0.f, s2 = 0.f;
  for (int z = 0; z < RS; ++z) { s1 += part[((long)z * 2 + 0) * C + c]; s2 += part[((long)z * 2 + 1) * C + c]; }
  dbeta[c] = s1;
  dgamma[c] = s2;
}
// dx = gamma / sqrt(var + eps) * (g - dbeta / M - xhat * dgamma / M); assigned or accumulated into dx (row stride ldd)
__global__ void ft_bn_bwd_apply_kernel(const float *__restrict__ dy, const float *__restrict__ x, int ld, long M, int C,
                                       const float *__restrict__ mean, const float *__restrict__ var,
                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                       const float *__restrict__ dgamma, const float *__restrict__ dbeta,
                                       float *__restrict__ dx, int ldd, int accumulate) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= M * C) return;
  const long r = id / C;
  const int c = (int)(id - r * C);
  const float is = rsqrtf(var[c] + kEps), xh = (x[r * ld + c] - mean[c]) * is;
  const float g = gamma[c] * xh + beta[c] > 0.f ? dy[id] : 0.f;
  const float v = gamma[c] * is * (g - dbeta[c] / (float)M - xh * dgamma[c] / (float)M);
  float *o = dx + r * ldd + c;
  *o = accumulate ? *o + v : v;
}
__global__ void ft_bn_running_kernel(float *__restrict__ rmean, float *__restrict__ rvar, const float *__restrict__ mean,
                                     const float *__restrict__ var, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  rmean[c] = kBnMom * rmean[c] + (1.f - kBnMom) * mean[c];
  rvar[c] = kBnMom * rvar[c] + (1.f - kBnMom) * var[c];
}

// ---- pools ------------------------------------------------------------------------------------------------------------
// maxpool 3x3 stride 2 pad 1: a (B,H,W,C) -> y rows of stride ldy
__global__ void ft_maxpool_kernel(const float *__restrict__ a, int B, int H, int W, int C, float *__restrict__ y, int ldy) {
  const int Ho = H / 2, Wo = W / 2;
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)B * Ho * Wo * C) return;
  const int c = (int)(id % C);
  const long m = id / C;
  const int ox = (int)(m % Wo), oy = (int)((m / Wo) % Ho), b = (int)(m / ((long)Wo * Ho));
  float best = -INFINITY;
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx) {
      const int iy = oy * 2 - 1 + ky, ix = ox * 2 - 1 + kx;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) best = fmaxf(best, a[(((long)b * H + iy) * W + ix) * C + c]);
    }
  y[m * ldy + c] = best;
}
// gradient of the maxpool (first maximum of the window in scan order takes it), gather form over the <= 4 windows of a pixel
__global__ void ft_maxpool_bwd_kernel(const float *__restrict__ a, const float *__restrict__ dy, int ldy, int B, int H, int W,
                                      int C, float *__restrict__ da) {
  const int Ho = H / 2, Wo = W / 2;
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)B * H * W * C) return;
  const int c = (int)(id % C);
  const long m = id / C;
  const int x = (int)(m % W), y = (int)((m / W) % H), b = (int)(m / ((long)W * H));
  float acc = 0.f;
  for (int oy = (y + 1) / 2 - ((y + 1) % 2 == 0 ? 1 : 0); oy <= (y + 1) / 2; ++oy)
    for (int ox = (x + 1) / 2 - ((x + 1) % 2 == 0 ? 1 : 0); ox <= (x + 1) / 2; ++ox) {
      if (oy < 0 || oy >= Ho || ox < 0 || ox >= Wo) continue;
      float best = -INFINITY;
      int by = -1, bx = -1;
      for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
          const int iy = oy * 2 - 1 + ky, ix = ox * 2 - 1 + kx;
          if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            const float v = a[(((long)b * H + iy) * W + ix) * C + c];
            if (v > best) { best = v; by = iy; bx = ix; }
          }
        }
      if (by == y && bx == x) acc += dy[(((long)b * Ho + oy) * Wo + ox) * ldy + c];
    }
  da[id] = acc;
}
// avgpool 2x2 stride 2: z (B,H,W,C) -> y rows of stride ldy ; and its gradient (dy rows of stride ldy -> dz contiguous)
__global__ void ft_avgpool2_kernel(const float *__restrict__ z, int B, int H, int W, int C, float *__restrict__ y, int ldy) {
  const int Ho = H / 2, Wo = W / 2;
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)B * Ho * Wo * C) return;
  const int c = (int)(id % C);
  const long m = id / C;
  const int ox = (int)(m % Wo), oy = (int)((m / Wo) % Ho), b = (int)(m / ((long)Wo * Ho));
  const float *p = z + (((long)b * H + 2 * oy) * W + 2 * ox) * C + c;
  y[m * ldy + c] = 0.25f * (p[0] + p[C] + p[(long)W * C] + p[(long)W * C + C]);
}
__global__ void ft_avgpool2_bwd_kernel(const float *__restrict__ dy, int ldy, int B, int H, int W, int C, float *__restrict__ dz) {
  const int Ho = H / 2, Wo = W / 2;
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)B * H * W * C) return;
  const int c = (int)(id % C);
  const long m = id / C;
  const int x = (int)(m % W), y = (int)((m / W) % H), b = (int)(m / ((long)W * H));
  dz[id] = 0.25f * dy[(((long)b * Ho + y / 2) * Wo + x / 2) * ldy + c];
}
// global average pool over the P pixels of a frame: a (B,P,C) -> f (B,C); gradient: da = df / P
__global__ void ft_gap_kernel(const float *__restrict__ a, int B, int P, int C, float *__restrict__ f) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= B * C) return;
  const int b = id / C, c = id - b * C;
  float s = 0.f;
  for (int p = 0; p < P; ++p) s += a[((long)b * P + p) * C + c];
  f[id] = s / (float)P;
}
__global__ void ft_gap_bwd_kernel(const float *__restrict__ df, int B, int P, int C, float *__restrict__ da) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)B * P * C) return;
  const int c = (int)(id % C);
  const int b = (int)(id / ((long)P * C));
  da[id] = df[(long)b * C + c] / (float)P;
}

inline unsigned nblk(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

// (the network's BatchNorms, layers and offsets: FtNet of param_table.h, filled by ft_param_table)
struct tn_finetune : TrainParams, FtNet {
  int B, H, W, classes;
  bool dense;                   // false: the backbone alone (the CNN-RNN step's TimeDistributed part), no classifier
  float *mom;                   // momentum, next to the parameters w, the gradients g and the running statistics in state
  float *av = nullptr;          // Adam's second moment (mom holds the first): ft_enable_adam
  int Hb[4];
  // activations kept for backward
  float *x_in, *col7, *z0, *a0, *X[4], *dX[4], *feat, *logits, *loss, *dlog, *dfeat;
  // batch statistics of every channel of a block's concat buffer, computed ONCE when the channel is produced: the BatchNorms in
  // front of the block's 1x1 convolutions, of its transition and of the head all normalise prefixes of the same channels
  float *Xmean[4], *Xvar[4];
  // temporaries
  float *ta, *tb, *col, *dcol, *tg, *tw, *ws;      // ws: split-K partial results / BatchNorm reduction slices
  long ws_floats;
  int32_t *labels;
  int matmul = TN_MATMUL_F32;   // which matrix pipe the backbone's GEMMs run on (tn_finetune_set_matmul), changeable between steps
  int64_t n_f32 = 0, n_x3 = 0;  // backbone GEMM launches per mode since creation (tn_finetune_matmul_stats)
};

// sc = gamma / sqrt(var + eps), sh = beta - mean * sc
__global__ void ft_bn_fold_kernel(const float *__restrict__ mean, const float *__restrict__ var, const float *__restrict__ gamma,
                                  const float *__restrict__ beta, int C, float *__restrict__ sc, float *__restrict__ sh) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float s = gamma[c] * rsqrtf(var[c] + kEps);
  sc[c] = s;
  sh[c] = fmaf(-mean[c], s, beta[c]);
}
static int ft_slices(long M, int C) {
  const int cb = (C + 63) / 64;
  int RS = (int)((M + 2047) / 2048);                 // >= 2048 rows per slice, <= 512 workgroups
  if (RS > 512 / cb) RS = 512 / cb;
  return RS < 1 ? 1 : RS;
}
// The training-mode BatchNorm launchers (train.h), on raw device pointers: what the step calls and what tn_dbg_bn_train runs.
// ws: at least ft_bn_ws_floats(M, C) floats of reduction slices.  (A launch error is peeked at, not cleared: the step checks once at its end.)
long ft_bn_ws_floats(long M, int C) { return (2L * ft_slices(M, C) + 1) * C; }
int launch_ft_bn_stats(const float *x, int ld, long M, int C, float *ws, float *mean, float *var, hipStream_t s) {
  const int RS = ft_slices(M, C);
  hipLaunchKernelGGL(ft_bn_stats_kernel, dim3((C + 63) / 64, RS), dim3(1024), 0, s, x, ld, M, C, ws);
  hipLaunchKernelGGL(ft_bn_stats_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (const float *)ws, RS, C, M, mean, var);
  TN_HIP_CHECK(hipPeekAtLastError());
  return TN_OK;
}
int launch_ft_bn_relu(const float *x, int ld, long M, int C, const float *mean, const float *var, const float *gamma, const float *beta,
                      float *y, hipStream_t s) {
  hipLaunchKernelGGL(ft_bn_relu_kernel, dim3(nblk(M * C)), dim3(256), 0, s, x, ld, M, C, mean, var, gamma, beta, y);
  TN_HIP_CHECK(hipPeekAtLastError());
  return TN_OK;
}
int launch_ft_bn_backward(const float *dy, const float *x, int ld, long M, int C, const float *mean, const float *var, const float *gamma,
                          const float *beta, float *ws, float *dgamma, float *dbeta, float *dx, int ldd, int accumulate, hipStream_t s) {
  const int cb = (C + 63) / 64, RS = ft_slices(M, C);
  hipLaunchKernelGGL(ft_bn_bwd_reduce_kernel, dim3(cb, RS), dim3(1024), 0, s, dy, x, ld, M, C, mean, var, gamma, beta, ws);
  hipLaunchKernelGGL(ft_bn_bwd_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (const float *)ws, RS, C, dgamma, dbeta);
  hipLaunchKernelGGL(ft_bn_bwd_apply_kernel, dim3(nblk(M * C)), dim3(256), 0, s, dy, x, ld, M, C, mean, var, gamma, beta,
                     (const float *)dgamma, (const float *)dbeta, dx, ldd, accumulate);
  TN_HIP_CHECK(hipPeekAtLastError());
  return TN_OK;
}
// The step's other operators (train.h), on raw device pointers: what the step calls and what the tn_dbg_ft_* hooks run, so the
// grid arithmetic is the step's.  Shapes are the kernels' (above); a launch error is peeked at, not cleared.
#define FT_LAUNCHED() do { TN_HIP_CHECK(hipPeekAtLastError()); return TN_OK; } while (0)
int launch_ft_im2col7(const float *x, int B, int H, int W, float *col, hipStream_t s) {
  hipLaunchKernelGGL(ft_im2col7_kernel, dim3(nblk((long)B * (H / 2) * (W / 2) * 49)), dim3(256), 0, s, x, B, H, W, col);
  FT_LAUNCHED();
}
int launch_ft_im2col3(const float *a, int B, int H, int W, int C, float *col, const float *sc, const float *sh, hipStream_t s) {
  hipLaunchKernelGGL(ft_im2col3_kernel, dim3(nblk((long)B * H * W * 9 * (C / 4))), dim3(256), 0, s, a, B, H, W, C, col, sc, sh);
  FT_LAUNCHED();
}
int launch_ft_col2im3(const float *dcol, int B, int H, int W, int C, float *da, hipStream_t s) {
  hipLaunchKernelGGL(ft_col2im3_kernel, dim3(nblk((long)B * H * W * (C / 4))), dim3(256), 0, s, dcol, B, H, W, C, da);
  FT_LAUNCHED();
}
int launch_ft_maxpool(const float *a, int B, int H, int W, int C, float *y, int ldy, hipStream_t s) {
  hipLaunchKernelGGL(ft_maxpool_kernel, dim3(nblk((long)B * (H / 2) * (W / 2) * C)), dim3(256), 0, s, a, B, H, W, C, y, ldy);
  FT_LAUNCHED();
}
int launch_ft_maxpool_bwd(const float *a, const float *dy, int ldy, int B, int H, int W, int C, float *da, hipStream_t s) {
  hipLaunchKernelGGL(ft_maxpool_bwd_kernel, dim3(nblk((long)B * H * W * C)), dim3(256), 0, s, a, dy, ldy, B, H, W, C, da);
  FT_LAUNCHED();
}
int launch_ft_avgpool2(const float *z, int B, int H, int W, int C, float *y, int ldy, hipStream_t s) {
  hipLaunchKernelGGL(ft_avgpool2_kernel, dim3(nblk((long)B * (H / 2) * (W / 2) * C)), dim3(256), 0, s, z, B, H, W, C, y, ldy);
  FT_LAUNCHED();
}
int launch_ft_avgpool2_bwd(const float *dy, int ldy, int B, int H, int W, int C, float *dz, hipStream_t s) {
  hipLaunchKernelGGL(ft_avgpool2_bwd_kernel, dim3(nblk((long)B * H * W * C)), dim3(256), 0, s, dy, ldy, B, H, W, C, dz);
  FT_LAUNCHED();
}
int launch_ft_gap(const float *a, int B, int P, int C, float *f, hipStream_t s) {
  hipLaunchKernelGGL(ft_gap_kernel, dim3(nblk((long)B * C)), dim3(256), 0, s, a, B, P, C, f);
  FT_LAUNCHED();
}
int launch_ft_gap_bwd(const float *df, int B, int P, int C, float *da, hipStream_t s) {
  hipLaunchKernelGGL(ft_gap_bwd_kernel, dim3(nblk((long)B * P * C)), dim3(256), 0, s, df, B, P, C, da);
  FT_LAUNCHED();
}
int launch_ft_bn_fold(const float *mean, const float *var, const float *gamma, const float *beta, int C, float *sc, float *sh, hipStream_t s) {
  hipLaunchKernelGGL(ft_bn_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, s, mean, var, gamma, beta, C, sc, sh);
  FT_LAUNCHED();
}
int launch_ft_bn_running(float *rmean, float *rvar, const float *mean, const float *var, int C, hipStream_t s) {
  hipLaunchKernelGGL(ft_bn_running_kernel, dim3((C + 255) / 256), dim3(256), 0, s, rmean, rvar, mean, var, C);
  FT_LAUNCHED();
}
#undef FT_LAUNCHED
static void ft_bn_forward(tn_finetune *f, const FtBn &bn, const float *x, int ld, long M, float *y, hipStream_t s) {
  (void)launch_ft_bn_stats(x, ld, M, bn.C, f->ws, bn.mean, bn.var, s);
  (void)launch_ft_bn_relu(x, ld, M, bn.C, bn.mean, bn.var, f->w + bn.o_gamma, f->w + bn.o_beta, y, s);
}
// batch statistics of columns [0, C) of x into mean / var (no BatchNorm attached: the shared per-channel statistics of a block)
static void ft_stats(tn_finetune *f, const float *x, int ld, long M, int C, float *mean, float *var, hipStream_t s) {
  (void)launch_ft_bn_stats(x, ld, M, C, f->ws, mean, var, s);
}
// relu(x * sc + sh) of a BatchNorm whose batch statistics are known (bn.mean / bn.var)
static void ft_bn_fold(tn_finetune *f, const FtBn &bn, hipStream_t s) {
  (void)launch_ft_bn_fold(bn.mean, bn.var, f->w + bn.o_gamma, f->w + bn.o_beta, bn.C, bn.sc, bn.sh, s);
}
static void ft_bn_recompute(tn_finetune *f, const FtBn &bn, const float *x, int ld, long M, float *y, hipStream_t s) {
  (void)launch_ft_bn_relu(x, ld, M, bn.C, bn.mean, bn.var, f->w + bn.o_gamma, f->w + bn.o_beta, y, s);
}
// dy (M,C) contiguous -> gradients of gamma / beta into f->g and dx (stride ldd), assigned or accumulated
static void ft_bn_backward(tn_finetune *f, const FtBn &bn, const float *dy, const float *x, int ld, long M, float *dx, int ldd,
                           int accumulate, hipStream_t s) {
  (void)launch_ft_bn_backward(dy, x, ld, M, bn.C, bn.mean, bn.var, f->w + bn.o_gamma, f->w + bn.o_beta, f->ws, f->g + bn.o_gamma,
                              f->g + bn.o_beta, dx, ldd, accumulate, s);
}

int ft_create(tn_ctx *ctx, const tn_param *params, int n_params, const char *backbone_prefix, const char *dense_prefix, int height,
              int width, int classes, int batch, tn_finetune **out, long *fit_frames) {
  tn_finetune *f = new tn_finetune();
  f->ctx = ctx; f->B = batch; f->H = height; f->W = width; f->dense = dense_prefix != nullptr; f->classes = f->dense ? classes : 0;
  f->table = ft_param_table(backbone_prefix, dense_prefix, classes, f);
  f->n = f->table.n;
  const int c = f->Ctot[3];
  auto fail = [&](int code) { f->pool.release(); delete f; return code; };
  std::vector<float> w, st;
  if (!f->table.load(ParamMap(params, n_params), w, st)) return fail(TN_ERR_MISSING);
  // device buffers (alloc: in P, for B frames; a dry pool only counts the bytes)
  auto alloc = [&](DevPool &P, long B) {
  auto fl = [&P](long n) { return P.alloc<float>((size_t)n); };
  f->w = fl(f->n); f->g = fl(f->n); f->mom = fl(f->n); f->state = fl(f->table.ns);
  const long M0 = B * (height / 2) * (width / 2);
  f->x_in = fl(B * height * width * 3); f->col7 = fl(M0 * 147); f->z0 = fl(M0 * 64); f->a0 = fl(M0 * 64);
  long maxMK = M0 * 64, maxM128 = 0;
  for (int b = 0; b < 4; ++b) {
    f->Hb[b] = height / (4 << b);
    const long M = B * f->Hb[b] * f->Hb[b];
    f->X[b] = fl(M * f->Ctot[b]); f->dX[b] = fl(M * f->Ctot[b]);
    for (auto &L : f->layers[b]) L.z1 = fl(M * 128);
    if (b < 3) f->trans[b].z = fl(M * f->trans[b].Cout);
    if (M * f->Ctot[b] > maxMK) maxMK = M * f->Ctot[b];
    if (M * 128 > maxM128) maxM128 = M * 128;
  }
  const long Mb0 = B * f->Hb[0] * f->Hb[0];
  f->ta = fl(maxMK); f->tb = fl(maxMK > maxM128 ? maxMK : maxM128); f->col = fl(Mb0 * 1152); f->dcol = fl(Mb0 * 1152);
  f->tg = fl(maxMK); f->tw = fl(1024L * 1024);
  f->ws_floats = 16L << 20; f->ws = fl(f->ws_floats);
  f->feat = fl(B * c); f->dfeat = fl(B * c);
  f->logits = f->loss = f->dlog = nullptr; f->labels = nullptr;
  if (f->dense) {
    f->logits = fl(B * classes); f->loss = fl(B); f->dlog = fl(B * classes);
    f->labels = (int32_t *)fl(B);                                 // (int32, the size of a float)
  }
  auto bnbuf = [&](FtBn &b) { b.mean = fl(b.C); b.var = fl(b.C); b.sc = fl(b.C); b.sh = fl(b.C); };
  // a BatchNorm over a prefix of a block's concat buffer reads the block's shared statistics
  auto bnshared = [&](FtBn &b, int blk) { b.mean = f->Xmean[blk]; b.var = f->Xvar[blk]; b.sc = fl(b.C); b.sh = fl(b.C); };
  for (int b = 0; b < 4; ++b) { f->Xmean[b] = fl(f->Ctot[b]); f->Xvar[b] = fl(f->Ctot[b]); }
  bnbuf(f->bn0); bnshared(f->bnF, 3);
  for (int b = 0; b < 4; ++b) {
    for (auto &L : f->layers[b]) { bnshared(L.bn1, b); bnbuf(L.bn2); }
    if (b < 3) bnshared(f->trans[b].bn, b);
  }
  };
  if (fit_frames) {
    // what batch frames need against what the device has free: the allocation is linear in the frames
    DevPool d1, d2;
    d1.dry = d2.dry = true;
    alloc(d1, 1); alloc(d2, 2);
    const long per = (long)(d2.bytes - d1.bytes), fixed = (long)d1.bytes - per;
    size_t freeb = 0, totalb = 0;
    TN_HIP_CHECK(hipMemGetInfo(&freeb, &totalb));
    const long avail = (long)(freeb - freeb / 20);                   // 5 % left to the runtime and other allocations
    if (fixed + per * (long)batch > avail) {
      *fit_frames = avail > fixed ? (avail - fixed) / per : 0;
      f->pool.release(); delete f;
      return TN_ERR_NOMEM;
    }
  }
  auto &P = f->pool;
  alloc(P, batch);
  if (P.failed) { tn_set_error("device allocation failed"); return fail(TN_ERR_NOMEM); }
  f->each_bn([&](FtBn &b) { f->table.set_ptr(b.name + "_batch_mean", b.mean); f->table.set_ptr(b.name + "_batch_var", b.var); });
  TN_HIP_CHECK(hipMemcpy(f->w, w.data(), sizeof(float) * f->n, hipMemcpyHostToDevice));
  TN_HIP_CHECK(hipMemcpy(f->state, st.data(), sizeof(float) * f->table.ns, hipMemcpyHostToDevice));
  TN_HIP_CHECK(hipMemset(f->g, 0, sizeof(float) * f->n));
  TN_HIP_CHECK(hipMemset(f->mom, 0, sizeof(float) * f->n));
  *out = f;
  return TN_OK;
}

extern "C" int tn_finetune_create(tn_ctx *ctx, const tn_param *params, int n_params, const char *backbone_prefix,
                                  const char *dense_prefix, int height, int width, int classes, int batch, tn_finetune **out) {
  TN_REQUIRE(ctx && params && backbone_prefix && dense_prefix && out, "tn_finetune_create: null argument");
  TN_REQUIRE(height > 0 && width > 0 && height % 32 == 0 && width % 32 == 0 && height == width && classes > 0 && batch > 0,
             "tn_finetune_create: frames must be square with a side divisible by 32");
  TN_ON_DEVICE(ctx->device);
  return ft_create(ctx, params, n_params, backbone_prefix, dense_prefix, height, width, classes, batch, out, nullptr);
}

// The backbone's GEMMs, one dispatch helper per form: the handle's matmul mode picks the f32 launchers (linear.hip, train.hip - the
// calls and arguments the step has always made) or their fp32x3 twins (gemm_fp32x3.hip), and the launch is counted.
// Y (M, N; ldy) = f(X) W^T, f the identity (sc == nullptr) or relu(x sc[k] + sh[k])
static int ft_linear(tn_finetune *f, const float *X, int ldx, const float *sc, const float *sh, const float *Wt, int ldw, float *Y, int ldy,
                     int M, int N, int K, hipStream_t s) {
  if (f->matmul == TN_MATMUL_FP32X3) {
    ++f->n_x3;
    return launch_linear_fp32x3(X, ldx, sc, sh, Wt, ldw, nullptr, Y, ldy, M, N, K, 0, s);
  }
  ++f->n_f32;
  if (sc) return launch_linear_f32_bnrelu(X, ldx, sc, sh, Wt, ldw, nullptr, Y, ldy, M, N, K, 0, s);
  return launch_linear_f32(X, ldx, Wt, ldw, nullptr, Y, ldy, M, N, K, 0, s);
}
// C (M, N; ldc) = A^T g(B) over K rows, g the identity (sc == nullptr) or relu(b sc[n] + sh[n]); split-K on the handle's workspace
static int ft_gemm_tn(tn_finetune *f, const float *A, int lda, const float *Bm, int ldb, const float *sc, const float *sh, float *Cm, int ldc,
                      int M, int N, int K, hipStream_t s) {
  if (f->matmul == TN_MATMUL_FP32X3) {
    ++f->n_x3;
    return launch_gemm_tn_fp32x3(A, lda, Bm, ldb, sc, sh, Cm, ldc, M, N, K, s, f->ws, f->ws_floats);
  }
  ++f->n_f32;
  if (sc) return launch_gemm_tn_f32_bnrelu(A, lda, Bm, ldb, sc, sh, Cm, ldc, M, N, K, s, f->ws, f->ws_floats);
  return launch_gemm_tn_f32(A, lda, Bm, ldb, Cm, ldc, M, N, K, s, f->ws, f->ws_floats);
}

extern "C" int tn_finetune_set_matmul(tn_finetune *f, int mode) {
  TN_REQUIRE(f, "tn_finetune_set_matmul: null handle");
  TN_REQUIRE(mode == TN_MATMUL_F32 || mode == TN_MATMUL_FP32X3, "tn_finetune_set_matmul: mode must be TN_MATMUL_F32 (0) or TN_MATMUL_FP32X3 (1)");
  f->matmul = mode;
  return TN_OK;
}
extern "C" int tn_finetune_matmul_stats(tn_finetune *f, int64_t *f32_launches, int64_t *fp32x3_launches) {
  TN_REQUIRE(f, "tn_finetune_matmul_stats: null handle");
  if (f32_launches) *f32_launches = f->n_f32;
  if (fp32x3_launches) *fp32x3_launches = f->n_x3;
  return TN_OK;
}

// The step in three parts (train.h), on the handle's stream; launch errors are peeked at by the launchers and checked once by the caller.
// Forward of x (B, H, W, 3) through the backbone in training mode, batch statistics of every BatchNorm -> ft_features (B, 1024 ...)
int ft_forward_features(tn_finetune *f, const float *x, int n) {
  TN_REQUIRE(n > 0 && n <= f->B, "ft_forward_features: the frames of a step must be between 1 and the handle's capacity");
  hipStream_t s = f->ctx->stream;
  const int B = n, H = f->H, W = f->W;
  const long M0 = (long)B * (H / 2) * (W / 2);
  float *w = f->w;
  TN_TRY(launch_ft_im2col7(x, B, H, W, f->col7, s));
  TN_TRY(ft_linear(f, f->col7, 147, nullptr, nullptr, w + f->o_w0, 147, f->z0, 64, (int)M0, 64, 147, s));
  ft_bn_forward(f, f->bn0, f->z0, 64, M0, f->a0, s);
  TN_TRY(launch_ft_maxpool(f->a0, B, H / 2, W / 2, 64, f->X[0], f->Ctot[0], s));
  // Round 4: (a) a channel's batch statistics are computed once, when it is produced (64 / 32 / Cout new columns at a time) - every
  // BatchNorm of the block that normalises it reads them; (b) BatchNorm + ReLU in front of a convolution is never stored: the 1x1
  // GEMMs transform their X operand while staging it (launch_linear_f32_bnrelu), im2col transforms the bottleneck on the way
  ft_stats(f, f->X[0], f->Ctot[0], (long)B * f->Hb[0] * f->Hb[0], f->Cin[0], f->Xmean[0], f->Xvar[0], s);
  for (int b = 0; b < 4; ++b) {
    const int Hh = f->Hb[b], Ct = f->Ctot[b];
    const long M = (long)B * Hh * Hh;
    for (auto &L : f->layers[b]) {
      ft_bn_fold(f, L.bn1, s);
      TN_TRY(ft_linear(f, f->X[b], Ct, L.bn1.sc, L.bn1.sh, w + L.o_w1, L.K, L.z1, 128, (int)M, 128, L.K, s));
      ft_stats(f, L.z1, 128, M, 128, L.bn2.mean, L.bn2.var, s);
      ft_bn_fold(f, L.bn2, s);
      TN_TRY(launch_ft_im2col3(L.z1, B, Hh, Hh, 128, f->col, L.bn2.sc, L.bn2.sh, s));
      TN_TRY(ft_linear(f, f->col, 1152, nullptr, nullptr, w + L.o_w3, 1152, f->X[b] + L.K, Ct, (int)M, 32, 1152, s));
      ft_stats(f, f->X[b] + L.K, Ct, M, 32, f->Xmean[b] + L.K, f->Xvar[b] + L.K, s);
    }
    if (b < 3) {
      FtTrans &T = f->trans[b];
      ft_bn_fold(f, T.bn, s);
      TN_TRY(ft_linear(f, f->X[b], Ct, T.bn.sc, T.bn.sh, w + T.o_w, T.Cin, T.z, T.Cout, (int)M, T.Cout, T.Cin, s));
      TN_TRY(launch_ft_avgpool2(T.z, B, Hh, Hh, T.Cout, f->X[b + 1], f->Ctot[b + 1], s));
      ft_stats(f, f->X[b + 1], f->Ctot[b + 1], M / 4, T.Cout, f->Xmean[b + 1], f->Xvar[b + 1], s);
    }
  }
  const int CF = f->Ctot[3], P3 = f->Hb[3] * f->Hb[3];
  const long M3 = (long)B * P3;
  ft_bn_recompute(f, f->bnF, f->X[3], CF, M3, f->ta, s);
  TN_TRY(launch_ft_gap(f->ta, B, P3, CF, f->feat, s));
  return TN_OK;
}

// Backward of the backbone from the feature gradient ft_feature_grad (B, 1024 ...): every backbone gradient, assigned
int ft_backward_features(tn_finetune *f, int n) {
  TN_REQUIRE(n > 0 && n <= f->B, "ft_backward_features: the frames of a step must be between 1 and the handle's capacity");
  hipStream_t s = f->ctx->stream;
  const int B = n, H = f->H, W = f->W;
  const long M0 = (long)B * (H / 2) * (W / 2);
  float *w = f->w, *g = f->g;
  const int CF = f->Ctot[3], P3 = f->Hb[3] * f->Hb[3];
  const long M3 = (long)B * P3;
  TN_TRY(launch_ft_gap_bwd(f->dfeat, B, P3, CF, f->tg, s));
  ft_bn_backward(f, f->bnF, f->tg, f->X[3], CF, M3, f->dX[3], CF, 0, s);
  for (int b = 3; b >= 0; --b) {
    const int Hh = f->Hb[b], Ct = f->Ctot[b];
    const long M = (long)B * Hh * Hh;
    for (int l = (int)f->layers[b].size() - 1; l >= 0; --l) {
      FtLayer &L = f->layers[b][l];
      const float *dy = f->dX[b] + L.K;                      // (M, 32) view, row stride Ct
      // 3x3: dW3 = dy^T col ; dcol = dy W3 ; col2im
      TN_TRY(launch_ft_im2col3(L.z1, B, Hh, Hh, 128, f->col, L.bn2.sc, L.bn2.sh, s));
      TN_TRY(ft_gemm_tn(f, dy, Ct, f->col, 1152, nullptr, nullptr, g + L.o_w3, 1152, 32, 1152, (int)M, s));
      TN_TRY(launch_transpose_f32(w + L.o_w3, 32, 1152, f->tw, s));                      // (1152, 32)
      TN_TRY(ft_linear(f, dy, Ct, nullptr, nullptr, f->tw, 32, f->dcol, 1152, (int)M, 1152, 32, s));
      TN_TRY(launch_ft_col2im3(f->dcol, B, Hh, Hh, 128, f->tg, s));
      ft_bn_backward(f, L.bn2, f->tg, L.z1, 128, M, f->tb, 128, 0, s);                  // tb = d z1
      // 1x1: dW1 = dz1^T a ; da = dz1 W1
      TN_TRY(ft_gemm_tn(f, f->tb, 128, f->X[b], Ct, L.bn1.sc, L.bn1.sh, g + L.o_w1, L.K, 128, L.K, (int)M, s));
      TN_TRY(launch_transpose_f32(w + L.o_w1, 128, L.K, f->tw, s));                     // (K, 128)
      TN_TRY(ft_linear(f, f->tb, 128, nullptr, nullptr, f->tw, 128, f->tg, L.K, (int)M, L.K, 128, s));
      ft_bn_backward(f, L.bn1, f->tg, f->X[b], Ct, M, f->dX[b], Ct, 1, s);               // accumulate into channels [0, K)
    }
    if (b > 0) {
      FtTrans &T = f->trans[b - 1];
      const int Hp = f->Hb[b - 1], Cp = f->Ctot[b - 1];
      const long Mp = (long)B * Hp * Hp;
      TN_TRY(launch_ft_avgpool2_bwd(f->dX[b], Ct, B, Hp, Hp, T.Cout, f->tb, s));
      TN_TRY(ft_gemm_tn(f, f->tb, T.Cout, f->X[b - 1], Cp, T.bn.sc, T.bn.sh, g + T.o_w, T.Cin, T.Cout, T.Cin, (int)Mp, s));
      TN_TRY(launch_transpose_f32(w + T.o_w, T.Cout, T.Cin, f->tw, s));                  // (Cin, Cout)
      TN_TRY(ft_linear(f, f->tb, T.Cout, nullptr, nullptr, f->tw, T.Cout, f->tg, T.Cin, (int)Mp, T.Cin, T.Cout, s));
      ft_bn_backward(f, T.bn, f->tg, f->X[b - 1], Cp, Mp, f->dX[b - 1], Cp, 0, s);
    } else {
      // stem: maxpool -> BN+ReLU -> conv 7x7 (its input gradient is not needed)
      ft_bn_recompute(f, f->bn0, f->z0, 64, M0, f->a0, s);
      TN_TRY(launch_ft_maxpool_bwd(f->a0, f->dX[0], Ct, B, H / 2, W / 2, 64, f->tg, s));
      ft_bn_backward(f, f->bn0, f->tg, f->z0, 64, M0, f->tb, 64, 0, s);
      TN_TRY(ft_gemm_tn(f, f->tb, 64, f->col7, 147, nullptr, nullptr, g + f->o_w0, 147, 64, 147, (int)M0, s));
    }
  }
  return TN_OK;
}

// BatchNorm running statistics from the batch statistics of the last forward: running = 0.9 running + 0.1 batch
void ft_update_running(tn_finetune *f) {
  hipStream_t s = f->ctx->stream;
  f->each_bn([&](const FtBn &b) {
    (void)launch_ft_bn_running(f->state + b.o_rm, f->state + b.o_rv, b.mean, b.var, b.C, s);
  });
}

float *ft_features(tn_finetune *f) { return f->feat; }
float *ft_feature_grad(tn_finetune *f) { return f->dfeat; }
int ft_feature_dim(tn_finetune *f) { return f->Ctot[3]; }
float *ft_frame_staging(tn_finetune *f) { return f->x_in; }
// gluon.Trainer(model.collect_params(), 'adam') covers the backbone inside the captioner too (reference train_gnmt.py:310)
int ft_enable_adam(tn_finetune *f) {
  if (f->av) return TN_OK;
  f->av = f->pool.alloc<float>(f->n);
  if (!f->av) { tn_set_error("device allocation failed"); return TN_ERR_NOMEM; }
  TN_HIP_CHECK(hipMemsetAsync(f->av, 0, sizeof(float) * f->n, f->ctx->stream));
  return TN_OK;
}
int ft_adam_step(tn_finetune *f, float lr, float beta1, float beta2, float epsilon, long step, const float *scale) {
  TN_REQUIRE(f->av, "ft_adam_step: ft_enable_adam has not run");
  return launch_adam(f->w, f->g, f->mom, f->av, f->n, lr, beta1, beta2, epsilon, step, f->ctx->stream, scale);
}
int ft_sgd_update(tn_finetune *f, float lr, float momentum, float wd, float rescale_grad, const float *scale) {
  return launch_sgd_momentum(f->w, f->g, f->mom, f->n, lr, momentum, wd, rescale_grad, f->ctx->stream, scale);
}
// x (batch, H, W, 3) fp32 normalised frames (NHWC), labels (batch,) int32, both DEVICE.  Runs the training-mode forward,
// the per-sample softmax cross-entropy and the backward of their SUM; loss (batch,) / logits (batch, classes) optional
// device outputs.  Gradients land in the flat buffer (tn_finetune_buffers); BatchNorm running statistics are updated.
extern "C" int tn_finetune_forward_backward(tn_finetune *f, const float *x, const int32_t *labels, int batch, int height, int width,
                                            float *loss, float *logits) {
  TN_REQUIRE(f && x && labels, "tn_finetune_forward_backward: null argument");
  TN_REQUIRE(height == f->H && width == f->W, "tn_finetune_forward_backward: the frame size must equal the handle's");
  TN_REQUIRE(batch == f->B, "tn_finetune_forward_backward: the batch must equal the handle's (BatchNorm statistics are per batch)");
  TN_REQUIRE(f->dense, "tn_finetune_forward_backward: the handle has no classifier");
  TN_ON_DEVICE(f->ctx->device);
  hipStream_t s = f->ctx->stream;
  const int B = f->B, NC = f->classes, CF = f->Ctot[3];
  float *w = f->w, *g = f->g;
  TN_TRY(ft_forward_features(f, x, B));
  TN_TRY(launch_linear_f32(f->feat, CF, w + f->o_wd, CF, w + f->o_bd, f->logits, NC, B, NC, CF, 0, s));
  TN_HIP_CHECK(hipMemcpyAsync(f->labels, labels, sizeof(int32_t) * B, hipMemcpyDeviceToDevice, s));
  TN_TRY(launch_softmax_ce(f->logits, f->labels, B, NC, f->loss, f->dlog, s));
  if (loss) TN_HIP_CHECK(hipMemcpyAsync(loss, f->loss, sizeof(float) * B, hipMemcpyDeviceToDevice, s));
  if (logits) TN_HIP_CHECK(hipMemcpyAsync(logits, f->logits, sizeof(float) * B * NC, hipMemcpyDeviceToDevice, s));
  TN_TRY(launch_dense_bwd(f->dlog, f->feat, w + f->o_wd, B, NC, CF, g + f->o_wd, g + f->o_bd, f->dfeat, s));
  TN_TRY(ft_backward_features(f, B));
  ft_update_running(f);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

extern "C" int tn_finetune_buffers(tn_finetune *f, float **params_dev, float **grads_dev, int64_t *numel) {
  return train_buffers("tn_finetune_buffers", f, params_dev, grads_dev, numel);
}

extern "C" int tn_finetune_sgd_step(tn_finetune *f, float lr, float momentum, float wd, float rescale_grad) {
  TN_REQUIRE(f, "tn_finetune_sgd_step: null handle");
  TN_ON_DEVICE(f->ctx->device);
  if (!f->clip.on()) return ft_sgd_update(f, lr, momentum, wd, rescale_grad, nullptr);
  if (int rc = f->clip.reduce(f->ctx, f->g, f->n, nullptr, 0, rescale_grad)) return rc;
  return ft_sgd_update(f, lr, momentum, wd, rescale_grad, f->clip.scale());
}

extern "C" int tn_finetune_set_clip(tn_finetune *f, float max_norm) {
  TN_REQUIRE(f, "tn_finetune_set_clip: null handle");
  return f->clip.set("tn_finetune_set_clip", f->ctx, max_norm);
}
extern "C" int tn_finetune_clip_stats(tn_finetune *f, float *norm, float *scale, int64_t *clipped_steps) {
  TN_REQUIRE(f, "tn_finetune_clip_stats: null handle");
  return f->clip.stats("tn_finetune_clip_stats", f->ctx, norm, scale, clipped_steps);
}

// Gluon-named parameter (conv weights back in (O, I, kh, kw) order), its gradient (gradient = 1), a running statistic, or
// a BatchNorm's batch statistic of the last step ("<bn>_batch_mean" / "<bn>_batch_var", test hook)
extern "C" int tn_finetune_read_param(tn_finetune *f, const char *name, int gradient, float *out_host, int64_t capacity, int64_t *numel) {
  return train_read_param("tn_finetune_read_param", f, name, gradient, out_host, capacity, numel);
}

extern "C" int tn_finetune_destroy(tn_finetune *f) {
  if (!f) return TN_OK;
  TnDeviceGuard tn_dg_(f->ctx->device);
  (void)hipStreamSynchronize(f->ctx->stream);
  f->clip.release();
  f->pool.release();
  delete f;
  return TN_OK;
}
