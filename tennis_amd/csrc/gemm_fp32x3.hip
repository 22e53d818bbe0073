// The fp32x3 training GEMMs: the two plain matrix products of the backbone training step (finetune.hip) with fp32 operands, fp32
// accumulators and fp32 results, the products on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16).  The recipe is the fp32x3
// encoder mode's (dense_fp32x3.hip): every fp32 operand value v is handed over as three bf16 terms
//   v1 = bf16(v),  v2 = bf16(v - v1),  v3 = bf16(v - v1 - v2)        (round to nearest even; the fp32 subtractions are exact)
// and of the nine cross products the six largest are formed, per 16-wide k-step and in this order, into ONE fp32 accumulator set:
//   a1 b1, a1 b2, a2 b1, a2 b2, a1 b3, a3 b1                        (dropped: a2 b3, a3 b2, a3 b3 <= 2^-24 |a||b|)
// with ascending k inside a split-K slice.  The order is the same for every tile shape, so an output value is the same bits
// whichever variant a launcher picks.  bf16 has fp32's exponent range: nothing is scaled.
// Non-finite input: as in the encoder mode, a value beyond bf16's largest finite number (3.39e38) rounds to infinity in v1 and
// its split is NaN; an infinity or a NaN in an operand gives NaN in every output it meets.
//
// Here BOTH operands change every step, so both are split in the loader, in registers (split2: v_cvt_pk_bf16_f32 and two exact
// subtractions per term), and written as three bf16 LDS planes [row][32 k]: 64-byte rows whose four 16-byte chunks are XOR-ed with
// (row >> 2) & 3, the encoder kernel's layout - the fragment read of the 32x32x16 operand map (lane l: row l & 31, k = 8 (l >> 5)
// + j, 16 bytes) is bank-conflict free without padding.  "row" is the operand's non-reduced index: an output row for the first
// operand, an output column for the second.
//   NT  (launch_linear_fp32x3):  Y = f(X) W^T.  Both operands have k contiguous: a loader slot is 8 consecutive k of one row.
//   TN  (launch_gemm_tn_fp32x3): C = A^T g(B).  The reduction index is the ROW of both operands in memory.  The transposing stage is
//       the loader itself: a slot is one column and 8 consecutive reduction rows, read as 8 dwords (the lanes of a wave take
//       consecutive columns: each load is one contiguous 256-byte segment), which is exactly the 16-byte k-chunk of that column's
//       LDS row after the split - the same planes, fragment reads and MFMA loop as the NT form.  The 16 lanes of a write group
//       hold 16 consecutive rows of one chunk, which the XOR spreads over the 16 slots of the 256-byte bank row.
// Padding contributes exactly 0: a k past K, a reduction row past the slice and a row / column past M or N are zero AFTER the
// operand transform (relu(0 sc + sh) is not 0), and nothing outside the operands' extents is read; stores go to [0, M) x [0, N).
// No float atomics: split-K slices go to the caller's workspace and are added in slice order.
#include "common.h"
#include "gemm_fp32x3.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kBK = 32;            // k per LDS stage: two 16-wide k-steps

// two fp32 values -> bf16 pair (round to nearest even), x in the low half          (dense_fp32x3.hip keeps its own copy: its
__device__ __forceinline__ unsigned cvt_pk_bf16(float x, float y) {              //  kernels' listings stay as they are)
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
__device__ __forceinline__ float relu_bn(float v, float s, float t) { return fmaxf(fmaf(v, s, t), 0.f); }

struct X3Args {
  const float *A, *B;        // NT: X (M, K; lda), W (N, K; ldb).  TN: A (K, lda) with M columns, B (K, ldb) with N columns
  long lda, ldb;
  const float *sc, *sh;      // NT: on A, per k.  TN: on B, per column n.  (BN instantiations only)
  const float *bias;         // NT only
  float *C;
  long ldc;
  int M, N, K;
  int accumulate;            // NT only
  int kchunk;                // TN: reduction rows per split-K slice (blockIdx.z), a multiple of kBK; slice z writes C + z M ldc
  int vecA, vecB;            // NT: the operand (and its sc / sh) can be read 16 bytes at a time
};

// WM x WN waves, each TM x TN fragments of 32 x 32: the tile is (32 WM TM) x (32 WN TN)
template <bool TNF, bool BN, int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(256) void gemm_fp32x3_kernel(const X3Args a) {
  static_assert(WM * WN == 4, "four waves");
  constexpr int BM = 32 * WM * TM, BN_ = 32 * WN * TN;
  constexpr int SA = BM * 4, SB = BN_ * 4;                  // loader slots (row, 8-k chunk) per stage
  constexpr int NA = (SA + 255) / 256, NB = (SB + 255) / 256;
  __shared__ uint4 As[3][SA];                               // [term][row][chunk ^ ((row >> 2) & 3)], a chunk = 8 k
  __shared__ uint4 Bs[3][SB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave / WN, wn = wave % WN;
  const long m0 = (long)blockIdx.x * BM, n0 = (long)blockIdx.y * BN_;      // rows on x: the stem has more row tiles than y holds
  // the reduction range of this workgroup
  const int kbeg = TNF ? (int)blockIdx.z * a.kchunk : 0;
  const int kend = TNF ? min(a.K, kbeg + a.kchunk) : a.K;
  float *Cout = a.C + (TNF ? (long)blockIdx.z * a.M * a.ldc : 0L);

  // slot i of this thread: NT row idx >> 2, chunk idx & 3 (a lane reads 32 contiguous bytes); TN row idx % rows, chunk idx / rows
  // (the lanes of a wave read consecutive columns of one reduction row)
  auto slot_row = [&](int idx, int rows) { return TNF ? idx % rows : idx >> 2; };
  auto slot_chunk = [&](int idx, int rows) { return TNF ? idx / rows : idx & 3; };

  float bsc[NB], bsh[NB];                                   // TN + BN: the slot's column transform
  if constexpr (TNF && BN) {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = tid + 256 * i;
      const long n = n0 + slot_row(idx, BN_);
      const bool ok = (SB % 256 == 0 || idx < SB) && n < a.N;
      bsc[i] = ok ? a.sc[n] : 0.f;
      bsh[i] = ok ? a.sh[n] : 0.f;
    }
  }

  // 8 values of one slot, transformed, zero wherever the operand ends
  auto load_a = [&](int i, int k0, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    const int idx = tid + 256 * i;
    if (SA % 256 != 0 && idx >= SA) return;
    const long m = m0 + slot_row(idx, BM);
    if (m >= a.M) return;
    const int k = k0 + 8 * slot_chunk(idx, BM);
    if constexpr (TNF) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (k + j < kend) v[j] = a.A[(long)(k + j) * a.lda + m];
    } else {
      const float *p = a.A + m * a.lda;
      if (a.vecA) {                                         // K % 4 == 0: a float4 is all inside or all outside
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int kk = k + 4 * h;
          if (kk < kend) {
            const float4 x = *(const float4 *)(p + kk);
            v[4 * h] = x.x; v[4 * h + 1] = x.y; v[4 * h + 2] = x.z; v[4 * h + 3] = x.w;
            if constexpr (BN) {
              const float4 s4 = *(const float4 *)(a.sc + kk), h4 = *(const float4 *)(a.sh + kk);
              v[4 * h] = relu_bn(v[4 * h], s4.x, h4.x); v[4 * h + 1] = relu_bn(v[4 * h + 1], s4.y, h4.y);
              v[4 * h + 2] = relu_bn(v[4 * h + 2], s4.z, h4.z); v[4 * h + 3] = relu_bn(v[4 * h + 3], s4.w, h4.w);
            }
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (k + j < kend) {
            v[j] = p[k + j];
            if constexpr (BN) v[j] = relu_bn(v[j], a.sc[k + j], a.sh[k + j]);
          }
      }
    }
  };
  auto load_b = [&](int i, int k0, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    const int idx = tid + 256 * i;
    if (SB % 256 != 0 && idx >= SB) return;
    const long n = n0 + slot_row(idx, BN_);
    if (n >= a.N) return;
    const int k = k0 + 8 * slot_chunk(idx, BN_);
    if constexpr (TNF) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (k + j < kend) {
          v[j] = a.B[(long)(k + j) * a.ldb + n];
          if constexpr (BN) v[j] = relu_bn(v[j], bsc[i], bsh[i]);
        }
    } else {
      const float *p = a.B + n * a.ldb;
      if (a.vecB) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int kk = k + 4 * h;
          if (kk < kend) {
            const float4 x = *(const float4 *)(p + kk);
            v[4 * h] = x.x; v[4 * h + 1] = x.y; v[4 * h + 2] = x.z; v[4 * h + 3] = x.w;
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (k + j < kend) v[j] = p[k + j];
      }
    }
  };
  float ra[NA][8], rb[NB][8];
#pragma unroll
  for (int i = 0; i < NA; ++i) load_a(i, kbeg, ra[i]);
#pragma unroll
  for (int i = 0; i < NB; ++i) load_b(i, kbeg, rb[i]);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

  for (int k0 = kbeg; k0 < kend; k0 += kBK) {
    __syncthreads();      // the previous stage has been read
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int idx = tid + 256 * i;
      if (SA % 256 == 0 || idx < SA) {
        const int row = slot_row(idx, BM);
        const int at = row * 4 + (slot_chunk(idx, BM) ^ ((row >> 2) & 3));
        uint4 p1, p2, p3;
        split2(ra[i][0], ra[i][1], p1.x, p2.x, p3.x);
        split2(ra[i][2], ra[i][3], p1.y, p2.y, p3.y);
        split2(ra[i][4], ra[i][5], p1.z, p2.z, p3.z);
        split2(ra[i][6], ra[i][7], p1.w, p2.w, p3.w);
        As[0][at] = p1; As[1][at] = p2; As[2][at] = p3;
      }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = tid + 256 * i;
      if (SB % 256 == 0 || idx < SB) {
        const int row = slot_row(idx, BN_);
        const int at = row * 4 + (slot_chunk(idx, BN_) ^ ((row >> 2) & 3));
        uint4 p1, p2, p3;
        split2(rb[i][0], rb[i][1], p1.x, p2.x, p3.x);
        split2(rb[i][2], rb[i][3], p1.y, p2.y, p3.y);
        split2(rb[i][4], rb[i][5], p1.z, p2.z, p3.z);
        split2(rb[i][6], rb[i][7], p1.w, p2.w, p3.w);
        Bs[0][at] = p1; Bs[1][at] = p2; Bs[2][at] = p3;
      }
    }
    __syncthreads();
    if (k0 + kBK < kend) {
#pragma unroll
      for (int i = 0; i < NA; ++i) load_a(i, k0 + kBK, ra[i]);
#pragma unroll
      for (int i = 0; i < NB; ++i) load_b(i, k0 + kBK, rb[i]);
    }
    // 32x32x16: lane l holds A[i = l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][j' = l & 31]
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[TM][3], bw[TN][3];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
        const int row = (wm * TM + tm) * 32 + (lane & 31);
        const int at = row * 4 + ((2 * ks + (lane >> 5)) ^ ((row >> 2) & 3));
#pragma unroll
        for (int p = 0; p < 3; ++p) af[tm][p] = __builtin_bit_cast(bf16x8, As[p][at]);
      }
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        const int row = (wn * TN + tn) * 32 + (lane & 31);
        const int at = row * 4 + ((2 * ks + (lane >> 5)) ^ ((row >> 2) & 3));
#pragma unroll
        for (int p = 0; p < 3; ++p) bw[tn][p] = __builtin_bit_cast(bf16x8, Bs[p][at]);
      }
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
      const long n = n0 + (wn * TN + tn) * 32 + (lane & 31);
      if (n >= a.N) continue;
      const float bz = (!TNF && a.bias) ? a.bias[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long m = m0 + (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= a.M) continue;
        float *dst = Cout + m * a.ldc + n;
        if constexpr (TNF) {
          *dst = acc[tm][tn][r];
        } else {
          const float v = acc[tm][tn][r] + bz;
          *dst = a.accumulate ? (*dst + v) : v;
        }
      }
    }
}

// sum of S (M, N) partial results (row stride N) into C (row stride ldc), slices added in order
__global__ void x3_splitk_reduce_kernel(const float *__restrict__ ws, int S, int M, int N, float *__restrict__ Cm, long ldc) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)M * N) return;
  float acc = 0.f;
  for (int z = 0; z < S; ++z) acc += ws[(long)z * M * N + id];
  Cm[(id / N) * ldc + id % N] = acc;
}

template <bool TNF, int WM, int WN, int TM, int TN>
int launch_tile(const X3Args &a, int slices, hipStream_t s) {
  const dim3 grid((unsigned)((a.M + 32 * WM * TM - 1) / (32 * WM * TM)), (unsigned)((a.N + 32 * WN * TN - 1) / (32 * WN * TN)), (unsigned)slices);
  TN_REQUIRE(grid.y <= 65535u && grid.z <= 65535u, "gemm_fp32x3: too many tiles for one launch");
  if (a.sc) hipLaunchKernelGGL((gemm_fp32x3_kernel<TNF, true, WM, WN, TM, TN>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((gemm_fp32x3_kernel<TNF, false, WM, WN, TM, TN>), grid, dim3(256), 0, s, a);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int launch_linear_fp32x3(const float *X, int ldx, const float *asc, const float *ash, const float *Wt, int ldw, const float *bias, float *Y,
                         int ldy, int M, int N, int K, int accumulate, hipStream_t s) {
  if (M <= 0 || N <= 0) return TN_OK;
  TN_REQUIRE((asc == nullptr) == (ash == nullptr), "linear_fp32x3: asc and ash go together");
  TN_REQUIRE(X && Wt && Y && K >= 0 && ldx >= K && ldw >= K && ldy >= N, "linear_fp32x3: null operand or a stride below its extent");
  X3Args a{};
  a.A = X; a.lda = ldx; a.B = Wt; a.ldb = ldw; a.sc = asc; a.sh = ash; a.bias = bias; a.C = Y; a.ldc = ldy;
  a.M = M; a.N = N; a.K = K; a.accumulate = accumulate; a.kchunk = K;
  a.vecA = ((ldx | K) & 3) == 0 && al16(X) && (!asc || (al16(asc) && al16(ash)));
  a.vecB = ((ldw | K) & 3) == 0 && al16(Wt);
  // tile shapes for the step's extremes: 32 output columns with a long K (3x3 forward), 64 (the stem), wide outputs with many rows
  // (1x1 forward, the input gradients), and few rows (block 4 of a small batch).  The product order is the same in all of them.
  if (N <= 32) return launch_tile<false, 4, 1, 1, 1>(a, 1, s);                                   // 128 x 32
  if (N <= 64) return launch_tile<false, 4, 1, 1, 2>(a, 1, s);                                   // 128 x 64
  if ((long)((M + 127) / 128) * ((N + 127) / 128) >= 256) return launch_tile<false, 2, 2, 2, 2>(a, 1, s);   // 128 x 128
  return launch_tile<false, 2, 2, 1, 1>(a, 1, s);                                                // 64 x 64
}

int launch_gemm_tn_fp32x3(const float *A, int lda, const float *Bm, int ldb, const float *bsc, const float *bsh, float *Cm, int ldc, int M,
                          int N, int K, hipStream_t s, float *ws, long ws_floats) {
  if (M <= 0 || N <= 0) return TN_OK;
  TN_REQUIRE((bsc == nullptr) == (bsh == nullptr), "gemm_tn_fp32x3: bsc and bsh go together");
  TN_REQUIRE(A && Bm && Cm && K >= 0 && lda >= M && ldb >= N && ldc >= N, "gemm_tn_fp32x3: null operand or a stride below its extent");
  // the split-K policy of the f32 launcher (train.hip gemm_tn_dispatch), on 64 x 64 tiles whatever tile runs: few output tiles and
  // a long reduction are split over workgroups, the partial results summed in slice order
  const int tiles = ((N + 63) / 64) * ((M + 63) / 64);
  int S = 1;
  if (ws && tiles < 256 && K >= 2048) {
    S = (512 + tiles - 1) / tiles;
    if (S > K / 512) S = K / 512;
    while (S > 1 && (long)S * M * N > ws_floats) --S;
  }
  X3Args a{};
  a.A = A; a.lda = lda; a.B = Bm; a.ldb = ldb; a.sc = bsc; a.sh = bsh; a.M = M; a.N = N; a.K = K;
  a.kchunk = K > 0 ? K : 1;
  if (S > 1) {
    a.kchunk = (((K + S - 1) / S) + kBK - 1) / kBK * kBK;
    S = (K + a.kchunk - 1) / a.kchunk;
  }
  if (S > 1) { a.C = ws; a.ldc = N; } else { S = 1; a.C = Cm; a.ldc = ldc; }
  int rc;
  // The slices above are counted for 64 x 64 tiles (>= 512 workgroups); a 128 x 128 tile would leave a quarter of them - measured at
  // 224 x 224 x 64: 14.9 ms for the 1x1 / transition weight gradients against the f32 kernel's 5.3 - so no tile is larger than that.
  if (M <= 32) rc = launch_tile<true, 1, 4, 1, 1>(a, S, s);            // 32 x 128: the 3x3 weight gradients
  else rc = launch_tile<true, 2, 2, 1, 1>(a, S, s);                    // 64 x 64: the stem, the 1x1 and transition weight gradients
  if (rc || S == 1) return rc;
  hipLaunchKernelGGL(x3_splitk_reduce_kernel, dim3((unsigned)(((long)M * N + 255) / 256)), dim3(256), 0, s, (const float *)ws, S, M, N, Cm,
                     (long)ldc);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}
