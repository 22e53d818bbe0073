// Training step of the temporal head: bi-GRU(hidden) over (B,T,F) features -> max over T ->
// Dense(classes) -> SoftmaxCrossEntropyLoss, backward and SGD(momentum, wd) — the frozen-backbone recipe of
// reference train.py:298-299 (gluon.Trainer 'sgd'), :324 (SoftmaxCrossEntropyLoss), :410-424 (record / backward /
// trainer.step(batch_size)) with models/vision/definitions.py:94-110 as the model.  fp32 throughout.
//
// The forward recurrence is rnn.hip's persistent kernel with its `save` output (r, z, n and the h2h candidate term per
// step; LSTM: i, f, g, o, c); its BPTT is rnn_bptt.hip; the weight gradients are three transposed GEMMs over all
// B*T rows afterwards.  This unit holds the rest of the step: pooling, cross-entropy, the dense backward, the GEMMs, the
// optimisers and clipping.
#include "common.h"
#include "train.h"

namespace {

__global__ void pool_max_arg_kernel(const float *__restrict__ x, int B, int T, int F, float *__restrict__ y,
                                    int32_t *__restrict__ arg) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)B * F) return;
  const int b = (int)(id / F), f = (int)(id % F);
  const float *p = x + (long)b * T * F + f;
  float best = p[0];
  int at = 0;
  for (int t = 1; t < T; ++t) {
    const float v = p[(long)t * F];
    if (v > best) { best = v; at = t; }      // first maximum takes the gradient
  }
  y[id] = best;
  arg[id] = at;
}

// per-sample loss -log softmax(logits)[label] (gluon SoftmaxCrossEntropyLoss, sparse labels) and d(sum loss)/dlogits
__global__ void softmax_ce_kernel(const float *__restrict__ logits, const int32_t *__restrict__ labels, int B, int C,
                                  float *__restrict__ loss, float *__restrict__ dlogits) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float *p = logits + (long)b * C;
  float m = p[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, p[c]);
  float sum = 0.f;
  for (int c = 0; c < C; ++c) sum += expf(p[c] - m);
  const float lse = m + logf(sum);
  const int lab = labels[b];
  loss[b] = lse - p[lab];
  for (int c = 0; c < C; ++c) dlogits[(long)b * C + c] = expf(p[c] - lse) - (c == lab ? 1.f : 0.f);
}

// Dense backward (tiny: B x C x K = 32 x 11 x 256): one thread per weight / per pooled element
__global__ void dense_bwd_kernel(const float *__restrict__ dlogits, const float *__restrict__ pooled,
                                 const float *__restrict__ wd, int B, int C, int K, float *__restrict__ dwd,
                                 float *__restrict__ dbd, float *__restrict__ dpooled) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id < C * K) {
    const int c = id / K, k = id - c * K;
    float a = 0.f;
    for (int b = 0; b < B; ++b) a = fmaf(dlogits[(long)b * C + c], pooled[(long)b * K + k], a);
    dwd[id] = a;
  }
  if (id < C) {
    float a = 0.f;
    for (int b = 0; b < B; ++b) a += dlogits[(long)b * C + id];
    dbd[id] = a;
  }
  if (id < B * K) {
    const int b = id / K, k = id - b * K;
    float a = 0.f;
    for (int c = 0; c < C; ++c) a = fmaf(dlogits[(long)b * C + c], wd[(long)c * K + k], a);
    dpooled[id] = a;
  }
}

__global__ void scatter_pool_grad_kernel(const float *__restrict__ dpooled, const int32_t *__restrict__ arg, int B,
                                         int T, int F, float *__restrict__ dseq) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)B * T * F) return;
  const int f = (int)(id % F);
  const long bt = id / F;
  const int t = (int)(bt % T), b = (int)(bt / T);
  dseq[id] = arg[(long)b * F + f] == t ? dpooled[(long)b * F + f] : 0.f;
}

// C[M][N] = A^T B, A [K][lda] (M columns), B [K][ldb] (N columns): the weight gradients dW = dG^T X over all B*T rows.
// Exact-f32 MFMA 16x16x4, 64x64 tile, 4 waves each 32x32.  Both operands are k-major in memory, which is what the
// fragments want (lane = (column, k)): rows of 64 columns are staged as they lie, no transposes.  kTnPD k-tiles of 16
// stay in flight in registers (the compiler does not overlap a plain load -> LDS -> MFMA loop by itself).
constexpr int kTnPD = 4;
// BNB: the B operand goes through relu(b * bsc[n] + bsh[n]) while it is staged (finetune.hip).
// GB (the temporal head trained from a feature table): row k of B is row clamp(brows[k], 0, bn_rows - 1) of the table Bm points to
// (row stride ldb).  The staged row changes with every k-tile, so a thread keeps the index of its next data fetch in a register,
// loaded kTnPD k-tiles before that fetch is issued: no data load waits on an index load inside the loop.  The clamp keeps every
// read inside the table whatever brows holds.  k-loop and MFMA order are those of the plain form.
// ZB (with GB; the captioner trained from a feature table): an index below 0 names a PAD row of a ragged clip - zeros are staged
// for it, as the zero-padded batch holds them, and nothing is read; an index >= bn_rows still clamps.  Pad k-rows stay in their
// k-tiles: which k's share an MFMA is unchanged, so the sum is that of the materialised operand bit for bit.
template <bool BNB = false, bool GB = false, bool ZB = false>
__global__ __launch_bounds__(256) void gemm_tn_f32_kernel(const float *__restrict__ A, int lda,
                                                          const float *__restrict__ Bm, int ldb,
                                                          float *__restrict__ Cm, int ldc, int M, int N, int K, int kchunk,
                                                          const float *__restrict__ bsc = nullptr, const float *__restrict__ bsh = nullptr,
                                                          const int32_t *__restrict__ brows = nullptr, int bn_rows = 0) {
  // split-K: slice blockIdx.z covers rows [z*kchunk, (z+1)*kchunk) and writes its own (M, N) partial result
  A += (long)blockIdx.z * kchunk * lda;
  if constexpr (GB) brows += (long)blockIdx.z * kchunk;       // a slice of a gathered B is a slice of its index array
  else Bm += (long)blockIdx.z * kchunk * ldb;
  Cm += (long)blockIdx.z * M * ldc;
  K = min(kchunk, K - (int)blockIdx.z * kchunk);
  __shared__ float As[2][16][64 + 4], Bs[2][16][64 + 4];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6, wm = wid >> 1, wn = wid & 1;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const int sk = t >> 4, sc = (t & 15) * 4;           // staging: k row, 4 columns
  const bool vec = ((lda | ldb) & 3) == 0 && (((uintptr_t)A | (uintptr_t)Bm) & 15) == 0 && m0 + 64 <= M && n0 + 64 <= N;
  const int nk = (K + 15) / 16;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[i][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float av[kTnPD][4], bv[kTnPD][4];
  int bidx[kTnPD];                  // GB: slot p holds the table row of the k-tile slot p fetches next
  auto row_of = [&](int it) {       // the table row this thread stages for k-tile `it` (0 past the end: never read)
    const int k = it * 16 + sk;
    if constexpr (ZB) {             // -1: a pad row, staged as zeros
      const int r = it < nk && k < K ? brows[k] : 0;
      return r < 0 ? -1 : min(r, bn_rows - 1);
    } else {
      return it < nk && k < K ? min(max(brows[k], 0), bn_rows - 1) : 0;
    }
  };
  auto fetch = [&](int it, float *a4, float *b4, int brow) {
    const int k = it * 16 + sk;
#pragma unroll
    for (int q = 0; q < 4; ++q) { a4[q] = 0.f; b4[q] = 0.f; }
    if (it >= nk || k >= K) return;
    const long bk = GB ? brow : k;            // the row of Bm staged for this k
    const bool brd = !ZB || brow >= 0;        // ZB: a pad row keeps the zeros
    if (vec) {
      if constexpr (ZB) {
        const float4 va = *(const float4 *)(A + (long)k * lda + m0 + sc);
        a4[0] = va.x; a4[1] = va.y; a4[2] = va.z; a4[3] = va.w;
        if (brd) {
          const float4 vb = *(const float4 *)(Bm + bk * ldb + n0 + sc);
          b4[0] = vb.x; b4[1] = vb.y; b4[2] = vb.z; b4[3] = vb.w;
        }
      } else {
        const float4 va = *(const float4 *)(A + (long)k * lda + m0 + sc), vb = *(const float4 *)(Bm + bk * ldb + n0 + sc);
        a4[0] = va.x; a4[1] = va.y; a4[2] = va.z; a4[3] = va.w;
        b4[0] = vb.x; b4[1] = vb.y; b4[2] = vb.z; b4[3] = vb.w;
      }
      if constexpr (BNB) {
        const float4 s4 = *(const float4 *)(bsc + n0 + sc), h4 = *(const float4 *)(bsh + n0 + sc);
        b4[0] = fmaxf(fmaf(b4[0], s4.x, h4.x), 0.f); b4[1] = fmaxf(fmaf(b4[1], s4.y, h4.y), 0.f);
        b4[2] = fmaxf(fmaf(b4[2], s4.z, h4.z), 0.f); b4[3] = fmaxf(fmaf(b4[3], s4.w, h4.w), 0.f);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (m0 + sc + q < M) a4[q] = A[(long)k * lda + m0 + sc + q];
        if ((!ZB || brd) && n0 + sc + q < N) {
          b4[q] = Bm[bk * ldb + n0 + sc + q];
          if constexpr (BNB) b4[q] = fmaxf(fmaf(b4[q], bsc[n0 + sc + q], bsh[n0 + sc + q]), 0.f);
        }
      }
    }
  };
  if constexpr (GB) {               // the indices of the first 2 kTnPD k-tiles are requested together, ahead of any data
    int first[kTnPD];
#pragma unroll
    for (int p = 0; p < kTnPD; ++p) { first[p] = row_of(p); bidx[p] = row_of(p + kTnPD); }
#pragma unroll
    for (int p = 0; p < kTnPD; ++p) fetch(p, av[p], bv[p], first[p]);
  } else {
#pragma unroll
    for (int p = 0; p < kTnPD; ++p) fetch(p, av[p], bv[p], 0);
  }
  for (int it0 = 0; it0 < nk; it0 += kTnPD) {
#pragma unroll
    for (int p = 0; p < kTnPD; ++p) {
      const int it = it0 + p;
      if (it < nk) {              // block-uniform
        const int buf = it & 1;
        *(float4 *)&As[buf][sk][sc] = make_float4(av[p][0], av[p][1], av[p][2], av[p][3]);
        *(float4 *)&Bs[buf][sk][sc] = make_float4(bv[p][0], bv[p][1], bv[p][2], bv[p][3]);
        if constexpr (GB) {
          fetch(it + kTnPD, av[p], bv[p], bidx[p]);
          bidx[p] = row_of(it + 2 * kTnPD);
        } else {
          fetch(it + kTnPD, av[p], bv[p], 0);
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int kq = ks * 4 + (lane >> 4);
          float a[2], b[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            a[i] = As[buf][kq][wm * 32 + i * 16 + (lane & 15)];
            b[i] = Bs[buf][kq][wn * 32 + i * 16 + (lane & 15)];
          }
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 2; ++q) acc[i][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[q], acc[i][q], 0, 0, 0);
        }
      }
    }
  }
  // D[i=m][j=n]: lane: n = lane&15, m = (lane>>4)*4 + r
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int n = n0 + wn * 32 + q * 16 + (lane & 15);
      if (n >= N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * 32 + i * 16 + (lane >> 4) * 4 + r;
        if (m < M) Cm[(long)m * ldc + n] = acc[i][q][r];
      }
    }
}

// sum of S (M, N) partial results (row stride N) into C (row stride ldc), slices added in order
__global__ void splitk_reduce_kernel(const float *__restrict__ ws, int S, int M, int N, float *__restrict__ Cm, int ldc) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)M * N) return;
  float a = 0.f;
  for (int z = 0; z < S; ++z) a += ws[(long)z * M * N + id];
  Cm[(id / N) * ldc + id % N] = a;
}

// column sums of A [rows][lda] (the bias gradients): 64 columns per workgroup, 16 row groups, 16 loads in flight,
// partials combined in a fixed order
__global__ __launch_bounds__(1024) void colsum_f32_kernel(const float *__restrict__ A, int lda, int rows, int cols,
                                                          float *__restrict__ out) {
  __shared__ float part[16][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
  float a = 0.f;
  if (c < cols) {
    int r = rg;
    for (; r + 15 * 16 < rows; r += 16 * 16) {
      float v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = A[(long)(r + i * 16) * lda + c];
#pragma unroll
      for (int i = 0; i < 16; ++i) a += v[i];
    }
    for (; r < rows; r += 16) a += A[(long)r * lda + c];
  }
  part[rg][threadIdx.x & 63] = a;
  __syncthreads();
  if (rg == 0 && c < cols) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += part[i][threadIdx.x];
    out[c] = s;
  }
}

// MXNet sgd_mom_update [EXT]: mom = momentum*mom - lr*(rescale*grad + wd*w); w += mom.  CLIP: on scale * grad, the scale read from
// the handle's clip record (grad_sumsq_finalize_kernel); the un-clipped instantiation never reads the pointer.
template <bool CLIP>
__global__ void sgd_momentum_kernel(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ mom,
                                    long n, float lr, float momentum, float wd, float rescale, const float *__restrict__ scale) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (CLIP) rescale *= *scale;
  const float m = momentum * mom[i] - lr * (rescale * g[i] + wd * w[i]);
  mom[i] = m;
  w[i] += m;
}

// MXNet Adam [EXT]: m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; w -= lr_t m / (sqrt(v) + eps), lr_t bias-corrected.  CLIP: g is
// scale * g, as above.
template <bool CLIP>
__global__ void trn_adam_kernel(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ m,
                                float *__restrict__ v, long n, float lr_t, float b1, float b2, float eps,
                                const float *__restrict__ scale) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float gi = CLIP ? *scale * g[i] : g[i];
  const float mi = b1 * m[i] + (1.f - b1) * gi, vi = b2 * v[i] + (1.f - b2) * gi * gi;
  m[i] = mi; v[i] = vi;
  w[i] -= lr_t * mi / (sqrtf(vi) + eps);
}

// ---- global-norm gradient clipping (gluon.utils.clip_global_norm [EXT]) ----
// Stage one of the sum of squares over up to two (pointer, count) segments.  A segment is split at its first 16-byte boundary:
// at most 3 head floats, a body of float4s, at most 3 tail floats.  The body is cut into chunks of TN_GRAD_SUMSQ_CHUNK floats;
// workgroup b of the TN_GRAD_SUMSQ_GRID walks chunks b, b + GRID, b + 2 GRID, ...; in a chunk thread t loads the float4s t, t + 256,
// t + 512, t + 768 (all four in flight) and adds their 16 squares to its one fp32 partial in index order.  Head and tail floats
// go one each to threads 0..2 and 64..66 of workgroup 0.  The 256 partials of a workgroup meet in a fixed tree (xor shuffles
// 32, 16, .., 1 inside a wave, then waves 0 + 1 + 2 + 3 through LDS); one float per workgroup lands in part[].  Nothing here
// depends on the order the workgroups run in.
__device__ __forceinline__ float sumsq_segment(const float *__restrict__ p, long n, float acc) {
  if (n <= 0) return acc;
  const long mis = (long)(((uintptr_t)p >> 2) & 3);                  // floats past a 16-byte boundary
  long head = mis ? 4 - mis : 0;
  if (head > n) head = n;
  const long body4 = (n - head) >> 2, tail = (n - head) & 3;
  const float4 *__restrict__ q = (const float4 *)(p + head);
  constexpr long C4 = TN_GRAD_SUMSQ_CHUNK / 4;
  for (long c0 = (long)blockIdx.x * C4; c0 < body4; c0 += (long)TN_GRAD_SUMSQ_GRID * C4) {
    float4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long i = c0 + threadIdx.x + j * TN_GRAD_SUMSQ_BLOCK;
      v[j] = i < body4 ? q[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc = fmaf(v[j].x, v[j].x, acc); acc = fmaf(v[j].y, v[j].y, acc);
      acc = fmaf(v[j].z, v[j].z, acc); acc = fmaf(v[j].w, v[j].w, acc);
    }
  }
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;
    if (t < head) acc = fmaf(p[t], p[t], acc);
    if (t >= 64 && t - 64 < tail) { const float x = p[head + 4 * body4 + (t - 64)]; acc = fmaf(x, x, acc); }
  }
  return acc;
}

__global__ __launch_bounds__(TN_GRAD_SUMSQ_BLOCK) void grad_sumsq_kernel(const float *__restrict__ a, long na,
                                                                         const float *__restrict__ b, long nb,
                                                                         float *__restrict__ part) {
  __shared__ float wave_sum[TN_GRAD_SUMSQ_BLOCK / 64];
  float acc = sumsq_segment(a, na, 0.f);
  acc = sumsq_segment(b, nb, acc);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// Stage two, one workgroup: thread t adds part[t], part[t + 256], ... in double, the 256 doubles meet in a fixed LDS tree, and
// thread 0 writes the record: norm = |rescale| sqrt(sum), scale = min(1, max_norm / (norm + 1e-8)) in fp32 as MXNet's NDArrays
// compute it (a NaN norm gives a NaN scale), clipped += scale < 1.  max_norm <= 0 (the debug hook): scale 1, nothing counted.
__global__ __launch_bounds__(256) void grad_sumsq_finalize_kernel(const float *__restrict__ part, int parts, float rescale,
                                                                  float max_norm, tn_clip_record *__restrict__ rec) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < parts; i += 256) s += (double)part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)(fabs((double)rescale) * sqrt(red[0]));
    float scale = 1.f;
    if (max_norm > 0.f) {
      const float q = max_norm / (norm + 1e-8f);
      scale = q < 1.f || q != q ? q : 1.f;
      if (scale < 1.f) rec->clipped += 1;
    }
    rec->sumsq = red[0];
    rec->norm = norm;
    rec->scale = scale;
  }
}

// The step's frame staging: y (B, T, frame floats) = x, with zeros (the Pad() value of the normalised tensor,
// utils/captioning.py:33) in the frame slots t >= valid_len[b], whose content in x is never read.  frame % 4 == 0.
// Grid (blocks over a frame's float4s, B * T).
__global__ void stage_frames_kernel(const float *__restrict__ x, const int32_t *__restrict__ valid_len, int T, long frame4,
                                    float *__restrict__ y) {
  const int slot = blockIdx.y, b = slot / T, t = slot % T;
  const bool pad = t >= valid_len[b];
  const float4 *src = (const float4 *)x + (long)slot * frame4;
  float4 *dst = (float4 *)y + (long)slot * frame4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < frame4; i += (long)gridDim.x * blockDim.x)
    dst[i] = pad ? make_float4(0.f, 0.f, 0.f, 0.f) : src[i];
}

__global__ void transpose_f32_kernel(const float *__restrict__ src, int rows, int cols, float *__restrict__ dst) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)rows * cols) return;
  const int r = (int)(i / cols), c = (int)(i % cols);
  dst[(long)c * rows + r] = src[i];
}

}  // namespace

#define TN_LAUNCH_CHECK() do { TN_HIP_CHECK(hipGetLastError()); return TN_OK; } while (0)

int launch_pool_max_arg(const float *x, int B, int T, int F, float *y, int32_t *arg, hipStream_t s) {
  hipLaunchKernelGGL(pool_max_arg_kernel, dim3(((long)B * F + 255) / 256), dim3(256), 0, s, x, B, T, F, y, arg);
  TN_LAUNCH_CHECK();
}
int launch_softmax_ce(const float *logits, const int32_t *labels, int B, int C, float *loss, float *dlogits,
                      hipStream_t s) {
  hipLaunchKernelGGL(softmax_ce_kernel, dim3((B + 63) / 64), dim3(64), 0, s, logits, labels, B, C, loss, dlogits);
  TN_LAUNCH_CHECK();
}
int launch_dense_bwd(const float *dlogits, const float *pooled, const float *wd, int B, int C, int K, float *dwd,
                     float *dbd, float *dpooled, hipStream_t s) {
  const int n = (C * K > B * K ? C * K : B * K);
  hipLaunchKernelGGL(dense_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, s, dlogits, pooled, wd, B, C, K, dwd, dbd,
                     dpooled);
  TN_LAUNCH_CHECK();
}
int launch_scatter_pool_grad(const float *dpooled, const int32_t *arg, int B, int T, int F, float *dseq, hipStream_t s) {
  hipLaunchKernelGGL(scatter_pool_grad_kernel, dim3(((long)B * T * F + 255) / 256), dim3(256), 0, s, dpooled, arg, B, T,
                     F, dseq);
  TN_LAUNCH_CHECK();
}
// C (M,N) = A^T B over K rows; bsc / bsh non-null: B -> relu(B * bsc[n] + bsh[n]) on the way in (a BatchNorm + ReLU that is never stored)
static int gemm_tn_dispatch(const float *A, int lda, const float *Bm, int ldb, const float *bsc, const float *bsh, float *Cm, int ldc, int M,
                            int N, int K, hipStream_t s, float *workspace, long workspace_floats) {
  const int32_t *const no_rows = nullptr;
  const int tiles = ((N + 63) / 64) * ((M + 63) / 64);
  // few output tiles and a long reduction (weight gradients over all pixels): split K over workgroups, partial results
  // in the caller's workspace, summed in slice order (deterministic)
  int S = 1;
  if (workspace && tiles < 256 && K >= 2048) {
    S = (512 + tiles - 1) / tiles;
    if (S > K / 512) S = K / 512;
    while (S > 1 && (long)S * M * N > workspace_floats) --S;
  }
  const bool bn = bsc != nullptr;
  if (S <= 1) {
    const dim3 grid((N + 63) / 64, (M + 63) / 64, 1);
    if (bn) hipLaunchKernelGGL(gemm_tn_f32_kernel<true>, grid, dim3(256), 0, s, A, lda, Bm, ldb, Cm, ldc, M, N, K, K, bsc, bsh, no_rows, 0);
    else hipLaunchKernelGGL(gemm_tn_f32_kernel<false>, grid, dim3(256), 0, s, A, lda, Bm, ldb, Cm, ldc, M, N, K, K, bsc, bsh, no_rows, 0);
    TN_LAUNCH_CHECK();
  }
  const int kchunk = (((K + S - 1) / S) + 15) / 16 * 16;
  S = (K + kchunk - 1) / kchunk;
  const dim3 grid((N + 63) / 64, (M + 63) / 64, S);
  if (bn) hipLaunchKernelGGL(gemm_tn_f32_kernel<true>, grid, dim3(256), 0, s, A, lda, Bm, ldb, workspace, N, M, N, K, kchunk, bsc, bsh, no_rows, 0);
  else hipLaunchKernelGGL(gemm_tn_f32_kernel<false>, grid, dim3(256), 0, s, A, lda, Bm, ldb, workspace, N, M, N, K, kchunk, bsc, bsh, no_rows, 0);
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(((long)M * N + 255) / 256), dim3(256), 0, s, (const float *)workspace, S, M, N, Cm, ldc);
  TN_LAUNCH_CHECK();
}
int launch_gemm_tn_f32(const float *A, int lda, const float *Bm, int ldb, float *Cm, int ldc, int M, int N, int K,
                       hipStream_t s, float *workspace, long workspace_floats) {
  return gemm_tn_dispatch(A, lda, Bm, ldb, nullptr, nullptr, Cm, ldc, M, N, K, s, workspace, workspace_floats);
}
int launch_gemm_tn_f32_bnrelu(const float *A, int lda, const float *Bm, int ldb, const float *bsc, const float *bsh, float *Cm, int ldc,
                              int M, int N, int K, hipStream_t s, float *workspace, long workspace_floats) {
  return gemm_tn_dispatch(A, lda, Bm, ldb, bsc, bsh, Cm, ldc, M, N, K, s, workspace, workspace_floats);
}
// C (M, N) = A^T G over K rows with G[k] = table[clamp(rows[k], 0, n_rows - 1)]: the B operand gathered from a table while it is
// staged.  One slice (no split-K), as launch_gemm_tn_f32 without a workspace: the same k order, the same result bit for bit.
int launch_gemm_tn_f32_rows(const float *A, int lda, const float *table, int ld, const int32_t *rows, int n_rows, float *Cm, int ldc,
                            int M, int N, int K, hipStream_t s) {
  TN_REQUIRE(table && rows && n_rows > 0 && ld >= N, "gemm_tn_f32_rows: needs a table of at least one row, ld >= N, and the row indices");
  const dim3 grid((N + 63) / 64, (M + 63) / 64, 1);
  hipLaunchKernelGGL((gemm_tn_f32_kernel<false, true>), grid, dim3(256), 0, s, A, lda, table, ld, Cm, ldc, M, N, K, K, (const float *)nullptr,
                     (const float *)nullptr, rows, n_rows);
  TN_LAUNCH_CHECK();
}
// ... with pad rows: rows[k] < 0 is a row of zeros (a batch zero-padded to its longest clip), rows[k] >= n_rows clamps to the last
// row.  Un-split; equals launch_gemm_tn_f32 (no workspace) on the materialised zero-padded B bit for bit.
int launch_gemm_tn_f32_padrows(const float *A, int lda, const float *table, int ld, const int32_t *rows, int n_rows, float *Cm, int ldc,
                               int M, int N, int K, hipStream_t s) {
  TN_REQUIRE(table && rows && n_rows > 0 && ld >= N, "gemm_tn_f32_padrows: needs a table of at least one row, ld >= N, and the row indices");
  const dim3 grid((N + 63) / 64, (M + 63) / 64, 1);
  hipLaunchKernelGGL((gemm_tn_f32_kernel<false, true, true>), grid, dim3(256), 0, s, A, lda, table, ld, Cm, ldc, M, N, K, K, (const float *)nullptr,
                     (const float *)nullptr, rows, n_rows);
  TN_LAUNCH_CHECK();
}
int launch_colsum_f32(const float *A, int lda, int rows, int cols, float *out, hipStream_t s) {
  hipLaunchKernelGGL(colsum_f32_kernel, dim3((cols + 63) / 64), dim3(1024), 0, s, A, lda, rows, cols, out);
  TN_LAUNCH_CHECK();
}
int launch_sgd_momentum(float *w, const float *g, float *mom, long n, float lr, float momentum, float wd,
                        float rescale, hipStream_t s, const float *scale) {
  const dim3 grid((n + 255) / 256), block(256);
  if (scale) hipLaunchKernelGGL(sgd_momentum_kernel<true>, grid, block, 0, s, w, g, mom, n, lr, momentum, wd, rescale, scale);
  else hipLaunchKernelGGL(sgd_momentum_kernel<false>, grid, block, 0, s, w, g, mom, n, lr, momentum, wd, rescale, scale);
  TN_LAUNCH_CHECK();
}
int launch_adam(float *w, const float *g, float *m, float *v, long n, float lr, float beta1, float beta2, float epsilon, long step,
                hipStream_t s, const float *scale) {
  const double c1 = 1.0 - pow((double)beta1, (double)step), c2 = 1.0 - pow((double)beta2, (double)step);
  const float lr_t = (float)((double)lr * sqrt(c2) / c1);
  const dim3 grid((n + 255) / 256), block(256);
  if (scale) hipLaunchKernelGGL(trn_adam_kernel<true>, grid, block, 0, s, w, g, m, v, n, lr_t, beta1, beta2, epsilon, scale);
  else hipLaunchKernelGGL(trn_adam_kernel<false>, grid, block, 0, s, w, g, m, v, n, lr_t, beta1, beta2, epsilon, scale);
  TN_LAUNCH_CHECK();
}
int launch_grad_sumsq(const float *a, long na, const float *b, long nb, float rescale, float max_norm, float *partials,
                      tn_clip_record *rec, hipStream_t s) {
  TN_REQUIRE(partials && rec && na >= 0 && nb >= 0 && (a || !na) && (b || !nb), "launch_grad_sumsq: bad argument");
  TN_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 3) == 0, "launch_grad_sumsq: the segments must be 4-byte aligned");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(TN_GRAD_SUMSQ_GRID), dim3(TN_GRAD_SUMSQ_BLOCK), 0, s, a, na, b, nb, partials);
  hipLaunchKernelGGL(grad_sumsq_finalize_kernel, dim3(1), dim3(256), 0, s, (const float *)partials, TN_GRAD_SUMSQ_GRID, rescale,
                     max_norm, rec);
  TN_LAUNCH_CHECK();
}
int launch_stage_frames(const float *x, const int32_t *valid_len, int B, int T, long frame_floats, float *y, hipStream_t s) {
  TN_REQUIRE(x && y && valid_len && B > 0 && T > 0 && frame_floats > 0 && frame_floats % 4 == 0 && (long)B * T <= 65535,
             "launch_stage_frames: bad shape");
  TN_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "launch_stage_frames: the frame buffers must be 16-byte aligned");
  const long f4 = frame_floats / 4;
  const unsigned gx = (unsigned)((f4 + 255) / 256 < 64 ? (f4 + 255) / 256 : 64);
  hipLaunchKernelGGL(stage_frames_kernel, dim3(gx, B * T), dim3(256), 0, s, x, valid_len, T, f4, y);
  TN_LAUNCH_CHECK();
}
int launch_transpose_f32(const float *src, int rows, int cols, float *dst, hipStream_t s) {
  hipLaunchKernelGGL(transpose_f32_kernel, dim3(((long)rows * cols + 255) / 256), dim3(256), 0, s, src, rows, cols, dst);
  TN_LAUNCH_CHECK();
}
