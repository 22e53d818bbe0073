// fp32 NN-layout product C (M, N) = A (M, K) B (K, N), both operands row-major, on the exact-f32 matrix instruction
// v_mfma_f32_16x16x4f32.  Its use: the input gradient of the bi-RNN head of the end-to-end CNN-RNN step,
// dX (B*T, F) = dGI (B*T, 2 G H) W_ih (2 G H, F), with W_ih in the layout the head already keeps (both directions stacked,
// row-major) - launch_linear_f32 wants W transposed and launch_gemm_tn_f32 wants A transposed.
// 64 x 64 tile, BK = 16, four waves of 32 x 32 (2 x 2 fragments); B's k-tile (16 rows x 64 columns, coalesced float4 rows) is
// staged transposed into LDS so that the fragment reads are linear_f32_kernel's (linear.hip).  One accumulator chain per output element in k order.
#include "common.h"
#include "train.h"

namespace {

constexpr int kNnPD = 4;   // k-tiles in flight per thread (registers) ahead of the one being multiplied

__global__ __launch_bounds__(256) void gemm_nn_f32_kernel(const float *__restrict__ A, int lda, const float *__restrict__ Bm, int ldb,
                                                          float *__restrict__ Cm, int ldc, int M, int N, int K, int accumulate) {
  __shared__ float As[2][64][17];
  __shared__ float Bs[2][64][17];      // [n][k]
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  // staging: A row t / 4, k (t % 4) * 4 ; B k-row t / 16, columns (t % 16) * 4
  const int arow = t >> 2, ak = (t & 3) * 4;
  const int bk = t >> 4, bc = (t & 15) * 4;
  const bool vec = ((lda | ldb | K | N) & 3) == 0 && (((uintptr_t)A | (uintptr_t)Bm) & 15) == 0;
  const int am = m0 + arow, bn = n0 + bc;
  const float *arow_p = A + (long)am * lda;
  const int nk = (K + 15) / 16;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  float av[kNnPD][4], bv[kNnPD][4];
  auto fetch = [&](int it, float *a4, float *b4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { a4[j] = 0.f; b4[j] = 0.f; }
    if (it >= nk) return;
    const int ka = it * 16 + ak, kb = it * 16 + bk;
    if (vec) {
      if (am < M && ka < K) { const float4 v = *(const float4 *)(arow_p + ka); a4[0] = v.x; a4[1] = v.y; a4[2] = v.z; a4[3] = v.w; }
      if (kb < K && bn < N) {
        const float4 v = *(const float4 *)(Bm + (long)kb * ldb + bn);
        b4[0] = v.x; b4[1] = v.y; b4[2] = v.z; b4[3] = v.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (am < M && ka + j < K) a4[j] = arow_p[ka + j];
        if (kb < K && bn + j < N) b4[j] = Bm[(long)kb * ldb + bn + j];
      }
    }
  };
#pragma unroll
  for (int p = 0; p < kNnPD; ++p) fetch(p, av[p], bv[p]);

  for (int it0 = 0; it0 < nk; it0 += kNnPD) {
#pragma unroll
    for (int p = 0; p < kNnPD; ++p) {
      const int it = it0 + p;
      if (it < nk) {              // block-uniform
        const int buf = it & 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          As[buf][arow][ak + j] = av[p][j];
          Bs[buf][bc + j][bk] = bv[p][j];
        }
        fetch(it + kNnPD, av[p], bv[p]);
        __syncthreads();          // one barrier per k-tile: the other buffer is still being read by slower waves
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int kq = ks * 4 + (lane >> 4);
          float a[2], b[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            a[i] = As[buf][wm * 32 + i * 16 + (lane & 15)][kq];
            b[i] = Bs[buf][wn * 32 + i * 16 + (lane & 15)][kq];
          }
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
      }
    }
  }
  // D[i=m][j=n]: lane: n = lane & 15, m = (lane >> 4) * 4 + r
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 32 + j * 16 + (lane & 15);
      if (n >= N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * 32 + i * 16 + (lane >> 4) * 4 + r;
        if (m < M) {
          float *dst = Cm + (long)m * ldc + n;
          *dst = accumulate ? *dst + acc[i][j][r] : acc[i][j][r];
        }
      }
    }
}

}  // namespace

int launch_gemm_nn_f32(const float *A, int lda, const float *Bm, int ldb, float *Cm, int ldc, int M, int N, int K, int accumulate,
                       hipStream_t s) {
  TN_REQUIRE(A && Bm && Cm && M > 0 && N > 0 && K > 0 && lda >= K && ldb >= N && ldc >= N, "launch_gemm_nn_f32: bad shape");
  TN_REQUIRE((M + 63) / 64 <= 65535, "launch_gemm_nn_f32: M exceeds the grid");
  hipLaunchKernelGGL(gemm_nn_f32_kernel, dim3((N + 63) / 64, (M + 63) / 64), dim3(256), 0, s, A, lda, Bm, ldb, Cm, ldc, M, N, K,
                     accumulate);
  TN_HIP_CHECK(hipPeekAtLastError());
  return TN_OK;
}
