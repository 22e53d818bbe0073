// The recurrent kernels' dot products (rnn.hip, rnn_bptt.hip), forward against h and BPTT against the pre-activation gradients.  Every
// form keeps one accumulator per (gate row, batch row) and walks k in ascending order: the sums are the same bits whichever form runs.
//
// rnn_dot_big, for blocks whose weight columns do not fit the registers: a thread's H
// weights are split three ways - KR in registers, KL in LDS ([k/4][row][4] floats: conflict-free 16-byte reads), the rest
// streamed with 16 loads in flight - and the vector x (LDS, the same for all lanes of a wave) is not read per FMA: a lane reads
// 16 bytes per 16 k-values (lane l holds x[k0 + 4 (l mod 4) + e], e = 0..3) and the FMAs take the operand through DPP
// quad_perm:[j,j,j,j] (v_fmac_f32_dpp: lane j of the quad, broadcast to the quad) - 4 x fewer LDS instructions than one
// broadcast ds_read_b128 per four FMAs, no extra VALU work.  One accumulator, k ascending: results do not depend on KR / KL.
#pragma once
#include <hip/hip_runtime.h>

#define TN_FMA_Q(ACC, HREG, W, J)                                                                              \
  asm volatile("v_fmac_f32_dpp %0, %1, %2 quad_perm:[" #J "," #J "," #J "," #J "] row_mask:0xf bank_mask:0xf"  \
               : "+v"(ACC) : "v"(HREG), "v"(W))
// 16 k-values k0 .. k0+15: WV(i) is the weight of k0 + i
#define TN_DOT16(ACC, HQ, WV)                                                                                          \
  do {                                                                                                                 \
    TN_FMA_Q(ACC, HQ.x, WV(0), 0);  TN_FMA_Q(ACC, HQ.y, WV(1), 0);  TN_FMA_Q(ACC, HQ.z, WV(2), 0);  TN_FMA_Q(ACC, HQ.w, WV(3), 0);   \
    TN_FMA_Q(ACC, HQ.x, WV(4), 1);  TN_FMA_Q(ACC, HQ.y, WV(5), 1);  TN_FMA_Q(ACC, HQ.z, WV(6), 1);  TN_FMA_Q(ACC, HQ.w, WV(7), 1);   \
    TN_FMA_Q(ACC, HQ.x, WV(8), 2);  TN_FMA_Q(ACC, HQ.y, WV(9), 2);  TN_FMA_Q(ACC, HQ.z, WV(10), 2); TN_FMA_Q(ACC, HQ.w, WV(11), 2);  \
    TN_FMA_Q(ACC, HQ.x, WV(12), 3); TN_FMA_Q(ACC, HQ.y, WV(13), 3); TN_FMA_Q(ACC, HQ.z, WV(14), 3); TN_FMA_Q(ACC, HQ.w, WV(15), 3);  \
  } while (0)

// the thread's weights KR .. KR+KL-1 into the LDS share (w_k = wcol[k * stride]; `row` of `nrows` threads)
template <int KR, int KL>
__device__ __forceinline__ void rnn_dot_fill_lds(float *wl, int nrows, int row, const float *__restrict__ wcol, long stride) {
  for (int k4 = 0; k4 < KL / 4; ++k4) {
    float4 v;
    v.x = wcol[(long)(KR + 4 * k4 + 0) * stride]; v.y = wcol[(long)(KR + 4 * k4 + 1) * stride];
    v.z = wcol[(long)(KR + 4 * k4 + 2) * stride]; v.w = wcol[(long)(KR + 4 * k4 + 3) * stride];
    *(float4 *)(wl + ((long)k4 * nrows + row) * 4) = v;
  }
}

// acc + sum over k < H of w_k x[k] (H % 16 == 0, x 16-byte aligned in LDS); lane4 = 4 * (lane & 3)
template <int KR, int KL>
__device__ __forceinline__ float rnn_dot_big(float acc, const float (&wr)[KR], const float *wl, int nrows, int row,
                                             const float *__restrict__ wcol, long stride, const float *x, int H, int lane4) {
  static_assert(KR % 16 == 0 && KL % 16 == 0, "whole 16-wide chunks of x");
#pragma unroll
  for (int k = 0; k < KR; k += 16) {
    const float4 hq = *(const float4 *)(x + k + lane4);
#define TN_WV(i) wr[k + (i)]
    TN_DOT16(acc, hq, TN_WV);
#undef TN_WV
  }
#pragma unroll
  for (int k = 0; k < KL; k += 16) {
    const float4 hq = *(const float4 *)(x + KR + k + lane4);
    float w[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 v = *(const float4 *)(wl + ((long)(k / 4 + i) * nrows + row) * 4);
      w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
#define TN_WV(i) w[i]
    TN_DOT16(acc, hq, TN_WV);
#undef TN_WV
  }
  for (int k = KR + KL; k < H; k += 16) {
    float w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = wcol[(long)(k + i) * stride];
    const float4 hq = *(const float4 *)(x + k + lane4);
#define TN_WV(i) w[i]
    TN_DOT16(acc, hq, TN_WV);
#undef TN_WV
  }
  return acc;
}

// The streamed form, NB batch rows against one weight column: acc[b] += sum over k < H of w_k x[b * xstride + k], w_k = wcol[k * stride]
// (H % 4 == 0, x 16-byte aligned in LDS).  The first KR weights are the caller's registers wr (loop-invariant over the steps), the rest
// is streamed with 16 loads in flight (batched by hand: the compiler otherwise waits for every group of four), then a 4-wide tail.
// Forward: acc starts at the bias, wcol a column of the k-major W_hh^T (stride G*H), x = h (xstride H).  BPTT: acc starts at 0, wcol a
// column of a gate block of W_hh (stride H), x = that block of the pre-activation gradients (xstride G*H).
template <int NB, int KR>
__device__ __forceinline__ void rnn_dot_stream(float (&acc)[NB], const float (&wr)[KR > 0 ? KR : 1], const float *__restrict__ wcol,
                                               int stride, const float *x, int xstride, int H) {
#pragma unroll
  for (int k = 0; k < KR; k += 4) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float4 xv = *(const float4 *)(x + b * xstride + k);
      acc[b] = fmaf(wr[k + 0], xv.x, acc[b]);
      acc[b] = fmaf(wr[k + 1], xv.y, acc[b]);
      acc[b] = fmaf(wr[k + 2], xv.z, acc[b]);
      acc[b] = fmaf(wr[k + 3], xv.w, acc[b]);
    }
  }
  int k = KR;
  for (; k + 16 <= H; k += 16) {
    float w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = wcol[(long)(k + i) * stride];
#pragma unroll
    for (int i = 0; i < 16; i += 4) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const float4 xv = *(const float4 *)(x + b * xstride + k + i);
        acc[b] = fmaf(w[i + 0], xv.x, acc[b]);
        acc[b] = fmaf(w[i + 1], xv.y, acc[b]);
        acc[b] = fmaf(w[i + 2], xv.z, acc[b]);
        acc[b] = fmaf(w[i + 3], xv.w, acc[b]);
      }
    }
  }
  for (; k < H; k += 4) {
    const float w0 = wcol[(long)(k + 0) * stride], w1 = wcol[(long)(k + 1) * stride];
    const float w2 = wcol[(long)(k + 2) * stride], w3 = wcol[(long)(k + 3) * stride];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float4 xv = *(const float4 *)(x + b * xstride + k);
      acc[b] = fmaf(w0, xv.x, acc[b]);
      acc[b] = fmaf(w1, xv.y, acc[b]);
      acc[b] = fmaf(w2, xv.z, acc[b]);
      acc[b] = fmaf(w3, xv.w, acc[b]);
    }
  }
}

// ... with two weight columns per thread (the wide kernels: nothing in registers), 16 values of each in flight.  Two forms side by side:
// forward reads ONE float4 of h per batch row for both columns, BPTT reads each column's own gate block xofs[r] - folding them would
// make forward load h twice or reorder BPTT's FMAs, and either changes the kernels' instruction streams.
template <int NB>
__device__ __forceinline__ void rnn_dot_stream2_shared(float (&acc)[2][NB], const float *const (&wcol)[2], long stride, const float *x,
                                                       int xstride, int H) {
  int k = 0;
  for (; k + 16 <= H; k += 16) {
    float w[2][16];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 16; ++i) w[r][i] = wcol[r][(long)(k + i) * stride];
#pragma unroll
    for (int i = 0; i < 16; i += 4) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const float4 xv = *(const float4 *)(x + b * xstride + k + i);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          acc[r][b] = fmaf(w[r][i + 0], xv.x, acc[r][b]);
          acc[r][b] = fmaf(w[r][i + 1], xv.y, acc[r][b]);
          acc[r][b] = fmaf(w[r][i + 2], xv.z, acc[r][b]);
          acc[r][b] = fmaf(w[r][i + 3], xv.w, acc[r][b]);
        }
      }
    }
  }
  for (; k < H; k += 4) {
    float w[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) w[r][i] = wcol[r][(long)(k + i) * stride];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float4 xv = *(const float4 *)(x + b * xstride + k);
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        acc[r][b] = fmaf(w[r][0], xv.x, acc[r][b]);
        acc[r][b] = fmaf(w[r][1], xv.y, acc[r][b]);
        acc[r][b] = fmaf(w[r][2], xv.z, acc[r][b]);
        acc[r][b] = fmaf(w[r][3], xv.w, acc[r][b]);
      }
    }
  }
}
template <int NB>
__device__ __forceinline__ void rnn_dot_stream2(float (&acc)[2][NB], const float *const (&wcol)[2], const float *x,
                                                const int (&xofs)[2], int xstride, int H) {
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[r][b] = 0.f;
  int k = 0;
  for (; k + 16 <= H; k += 16) {
    float w[2][16];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 16; ++i) w[r][i] = wcol[r][(long)(k + i) * H];
#pragma unroll
    for (int i = 0; i < 16; i += 4) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const float4 xv = *(const float4 *)(x + b * xstride + xofs[r] + k + i);
          acc[r][b] = fmaf(w[r][i + 0], xv.x, acc[r][b]);
          acc[r][b] = fmaf(w[r][i + 1], xv.y, acc[r][b]);
          acc[r][b] = fmaf(w[r][i + 2], xv.z, acc[r][b]);
          acc[r][b] = fmaf(w[r][i + 3], xv.w, acc[r][b]);
        }
      }
    }
  }
  for (; k < H; k += 4) {
    float w[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) w[r][i] = wcol[r][(long)(k + i) * H];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const float4 xv = *(const float4 *)(x + b * xstride + xofs[r] + k);
        acc[r][b] = fmaf(w[r][0], xv.x, acc[r][b]);
        acc[r][b] = fmaf(w[r][1], xv.y, acc[r][b]);
        acc[r][b] = fmaf(w[r][2], xv.z, acc[r][b]);
        acc[r][b] = fmaf(w[r][3], xv.w, acc[r][b]);
      }
    }
  }
}
