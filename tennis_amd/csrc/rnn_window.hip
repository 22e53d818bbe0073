// K9w/K11w — dense windowed evaluation of the temporal heads (reference evaluate.py --window W --temp_pool gru|lstm|mean|max over
// models/vision/definitions.py:66-69,94-96,106-107 and the window sampling of dataset.py:190-201).
//
// The windows of neighbouring samples overlap, and the i2h projection of a frame does not depend on the window that asks for it:
// the projection runs ONCE over the rows of the feature matrix (linear.hip), and the recurrent kernel below gathers, per sample
// and step, the projected row its window names.  Neither the (samples, T, F) windows nor the (samples, T, 2H) sequence exist in
// memory: the max over the steps (definitions.py:107) is kept per unit while the sequence is walked.
//
//   row(b, t) = clamp(centre[b] + (t - T/2) * stride, lo[b], hi[b])      (TennisSet.window_frames in units of matrix rows)
//   and then clamp(row, 0, rows - 1), unconditionally: no content of centre / lo / hi makes a kernel read outside its input.
//
// The TABLE form (TAB) of both kernels takes the rows from an index table instead (TennisSet.window_table: any sample layout):
//   row(b, t) = clamp(idx[b * T + t], 0, rows - 1)      (a negative entry is row 0, not a zero row)
#include "common.h"
#include "rnn_dot.h"
#include "rnn_window.h"

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ long window_row(int centre, int lo, int hi, int t, int T, int stride, int rows) {
  long r = (long)centre + (long)(t - T / 2) * stride;     // (64-bit: no content of the index arrays overflows)
  r = min(max(r, (long)lo), (long)hi);
  return min(max(r, 0L), (long)rows - 1);
}

// The recurrence of rnn_recurrent_kernel (rnn.hip): one workgroup = one direction x NB samples, all T steps; thread j owns gate
// row j of W_hh and runs the same ascending-k fmaf chain with one accumulator per sample (measured against that path on the same
// windows: LSTM logits bit-equal, GRU logits within 1.8e-7; tests/test_gpu_window_head.py records it).  What differs:
//   * the gi row of (sample, step) is gathered (window_row); the reverse direction walks t = T-1 .. 0; no valid_len;
//   * no sequence store: every (sample, unit) keeps the running maximum of h, started from the first step's value, and writes
//     pooled[b][dir*H + u] once;
//   * NB is a multiple of G where it can be (NB*H units over G*H threads: every thread then finishes exactly NB/G units per
//     step) and the step's gi values are requested BEFORE the dot product, so their latency hides behind it;
//   * DPP (H % 16 == 0): h is not read per FMA - a lane reads 16 bytes per 16 k-values and the FMAs take h through
//     quad_perm (rnn_dot.h), 4 x fewer LDS instructions; KR = 128 (H == 128): the thread's whole weight column lives in
//     registers for all T steps, nothing of W_hh is re-read.
// TAB: `centre` is the (B, T) row table, lo / hi / stride are not read.  The table adds a dependent load (index -> gi row) in front
// of the gi request, so the indices run one step ahead: step s requests its gi values through the index registers that step s - 1
// loaded (one register per unit the thread finishes) and then requests the indices of step s + 1; both requests are in flight
// behind the dot product, and the gi request at the top of a step never waits on an index load.
// ARG: every unit also keeps the window position t whose state its maximum was read from and writes steps[b][dir*H + u] next to
// pooled.  pooled is computed by the same expression either way; the position moves by comparison only - forward `hn > old`,
// reverse (t walks downwards) `hn >= old` - so that in both directions a tie goes to the smallest t, the first-maximum rule of
// pool_max_arg_kernel (train.hip).  Without ARG the kernel is the code it was: `steps` is the last argument and is never read.
template <int G, int NB, int KR, bool DPP, int MAXT, bool TAB, bool ARG>
__global__ __launch_bounds__(MAXT) void rnn_window_kernel(
    const float *__restrict__ gi, int ldgi, int rows,   // [rows][2*G*H] i2h + b_i2h of every row of the feature matrix
    const float *__restrict__ whT,                      // [2][H][G*H]
    const float *__restrict__ bh,                       // [2][G*H]
    const int32_t *__restrict__ centre, const int32_t *__restrict__ lo, const int32_t *__restrict__ hi,   // [B]
    float *__restrict__ pooled,                         // [B][2*H]
    int B, int T, int stride, int H,
    int32_t *__restrict__ steps) {                      // ARG: [B][2*H] window position of every unit's maximum

  static_assert(!DPP || KR % 16 == 0, "whole 16-wide h chunks");
  static_assert(DPP || KR == 0, "the register-resident prefix is part of the DPP form");
  constexpr int MI = (NB + G - 1) / G;     // units a thread finishes per step (NB*H units over G*H threads)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int GH = G * H;
  float *hs = lds;                 // [NB][H]
  float *gh = hs + NB * H;         // [NB][GH]
  float *cs = gh + NB * GH;        // [NB][H] (LSTM)
  const int j = threadIdx.x;       // gate row
  const int dir = blockIdx.y;
  const int b0 = blockIdx.x * NB;
  const float *wcol = whT + (long)dir * H * GH + j;
  const float bj = bh[dir * GH + j];
  float wr[KR > 0 ? KR : 1];
#pragma unroll
  for (int k = 0; k < KR; ++k) wr[k] = wcol[(long)k * GH];

  // the units this thread finishes: idx = j + m*GH -> (sample b0 + idx / H, unit idx % H)
  int cen[MI], wlo[MI], whi[MI];
  // TAB: byte offset of the row of unit 0's sample in the table (B * T < 2^30: the launcher checks); unit m belongs to the
  // sample m * G further on (idx / H = j / H + m * G): that distance and the step are uniform and go into the scalar base of the load
  int jb = 0, ju = 0;
  unsigned tab = 0;
  int gtab = 0;                    // ... and every unit of a thread is the same u = (j + m * GH) % H = j % H
  if constexpr (TAB) {
    jb = j / H, ju = j - jb * H;
    tab = (unsigned)(b0 + jb) * (unsigned)T * 4u;
    gtab = dir * GH + ju;
  }
  int nxt[MI];                     // TAB: the table entry of the step to come
  bool live[MI];
  float hmax[MI];
  int hstep[ARG ? MI : 1];
#pragma unroll
  for (int m = 0; m < MI; ++m) {
    if constexpr (ARG) hstep[m] = 0;
    const int idx = j + m * GH;
    const int bg = b0 + idx / H;
    live[m] = idx < NB * H && bg < B;
    if constexpr (TAB) {
      nxt[m] = live[m] ? *(const int32_t *)((const char *)centre + ((size_t)m * G * T + (dir ? T - 1 : 0)) * 4 + tab) : 0;
    } else {
      cen[m] = live[m] ? centre[bg] : 0;
      wlo[m] = live[m] ? lo[bg] : 0;
      whi[m] = live[m] ? hi[bg] : 0;
    }
    hmax[m] = 0.f;
  }
  for (int i = j; i < NB * H; i += GH) {
    hs[i] = 0.f;
    if (G == 4) cs[i] = 0.f;
  }
  __syncthreads();

  for (int s = 0; s < T; ++s) {
    const int t = dir ? T - 1 - s : s;
    // this step's input pre-activations of the units the thread finishes below (requested now, used after the barrier)
    float gq[MI][G];
    const int tn = dir ? max(t - 1, 0) : min(t + 1, T - 1);      // TAB: the step to come (the last step asks for its own again)
#pragma unroll
    for (int m = 0; m < MI; ++m) {
      if (live[m]) {
        const int u = (j + m * GH) % H;
        const float *g;
        if constexpr (TAB) {
          g = gi + ((long)min(max(nxt[m], 0), rows - 1) * ldgi + gtab);
          nxt[m] = *(const int32_t *)((const char *)centre + ((size_t)m * G * T + tn) * 4 + tab);
        } else {
          g = gi + window_row(cen[m], wlo[m], whi[m], t, T, stride, rows) * ldgi + dir * GH + u;
        }
#pragma unroll
        for (int e = 0; e < G; ++e) gq[m][e] = g[e * H];
      }
    }
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = bj;
    if constexpr (DPP) {
      const int lane4 = (j & 3) * 4;
#pragma unroll
      for (int k = 0; k < KR; k += 16) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const float4 hq = *(const float4 *)(hs + b * H + k + lane4);
#define TN_WV(i) wr[k + (i)]
          TN_DOT16(acc[b], hq, TN_WV);
#undef TN_WV
        }
      }
      for (int k = KR; k < H; k += 16) {
        float w[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = wcol[(long)(k + i) * GH];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const float4 hq = *(const float4 *)(hs + b * H + k + lane4);
#define TN_WV(i) w[i]
          TN_DOT16(acc[b], hq, TN_WV);
#undef TN_WV
        }
      }
    } else {
      int k = 0;
      for (; k + 16 <= H; k += 16) {
        float w[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = wcol[(long)(k + i) * GH];
#pragma unroll
        for (int i = 0; i < 16; i += 4) {
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            const float4 hv = *(const float4 *)(hs + b * H + k + i);
            acc[b] = fmaf(w[i + 0], hv.x, acc[b]);
            acc[b] = fmaf(w[i + 1], hv.y, acc[b]);
            acc[b] = fmaf(w[i + 2], hv.z, acc[b]);
            acc[b] = fmaf(w[i + 3], hv.w, acc[b]);
          }
        }
      }
      for (; k < H; k += 4) {
        const float w0 = wcol[(long)(k + 0) * GH], w1 = wcol[(long)(k + 1) * GH];
        const float w2 = wcol[(long)(k + 2) * GH], w3 = wcol[(long)(k + 3) * GH];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const float4 hv = *(const float4 *)(hs + b * H + k);
          acc[b] = fmaf(w0, hv.x, acc[b]);
          acc[b] = fmaf(w1, hv.y, acc[b]);
          acc[b] = fmaf(w2, hv.z, acc[b]);
          acc[b] = fmaf(w3, hv.w, acc[b]);
        }
      }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) gh[b * GH + j] = acc[b];
    __syncthreads();
#pragma unroll
    for (int m = 0; m < MI; ++m) {
      if (!live[m]) continue;
      const int idx = j + m * GH;
      int b, u;
      if constexpr (TAB) {
        // the same (b, u), from the thread's one division; the empty asm keeps the LDS addresses below from being hoisted out of
        // the step loop into registers of their own (with them the plain GRU form at NB = 6 went over its 128 registers into
        // scratch): a few integer instructions per step instead
        b = jb + m * G, u = ju;
        asm volatile("" : "+v"(b), "+v"(u));
      } else {
        b = idx / H, u = idx - b * H;
      }
      const float *q = gh + b * GH;
      float hn;
      if (G == 3) {
        const float r = sigmoidf_(gq[m][0] + q[u]);
        const float z = sigmoidf_(gq[m][1] + q[H + u]);
        const float n = tanhf(gq[m][2] + r * q[2 * H + u]);
        if constexpr (ARG) {
          // the form without ARG compiles this line to one packed multiply of both products and an add - two rounded products,
          // no fused multiply-add; with the comparisons below the compiler fuses instead, which moves the last bit of h.  The same
          // bits are the contract (tests/test_gpu_step_maps.py holds pooled to them), so the unfused form is spelt out here.
#pragma clang fp contract(off)
          hn = (1.f - z) * n + z * hs[idx];
        } else {
          hn = (1.f - z) * n + z * hs[idx];
        }
      } else {
        const float ig = sigmoidf_(gq[m][0] + q[u]);
        const float fg = sigmoidf_(gq[m][1] + q[H + u]);
        const float gg = tanhf(gq[m][2] + q[2 * H + u]);
        const float og = sigmoidf_(gq[m][G - 1] + q[3 * H + u]);
        const float c2 = fg * cs[idx] + ig * gg;
        cs[idx] = c2;
        hn = og * tanhf(c2);
      }
      hs[idx] = hn;
      if constexpr (ARG) {
        // one select on integer flags, no branch: as `if (s == 0 || (dir ? hn >= old : hn > old)) hstep = t` the streamed and plain
        // forms came out with the assignment outside its masked region (steps wrong on the GPU, pooled right)
        const int moved = (int)(s == 0) | (dir ? (int)(hn >= hmax[m]) : (int)(hn > hmax[m]));
        hstep[m] = moved ? t : hstep[m];
      }
      hmax[m] = s == 0 ? hn : fmaxf(hmax[m], hn);
    }
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < MI; ++m) {
    if (!live[m]) continue;
    const int idx = j + m * GH;
    const int b = idx / H, u = idx - b * H;
    pooled[(long)(b0 + b) * (2 * H) + dir * H + u] = hmax[m];
    if constexpr (ARG) steps[(long)(b0 + b) * (2 * H) + dir * H + u] = hstep[m];
  }
}

// F.max / F.mean over the gathered rows of the feature matrix itself (definitions.py:66-69 in feature mode), t ascending as in
// temporal_pool_kernel (rnn.hip): x (rows, F) -> y (B, F).  ARG (max only): arg (B, F) the first window position that holds the
// maximum (`v > old`: a tie stays with the smaller t, as in pool_max_arg_kernel); y is the same fmaxf chain either way.
template <bool TAB, bool ARG>
__global__ void temporal_pool_windows_kernel(const float *__restrict__ x, int rows, int F, const int32_t *__restrict__ centre,
                                             const int32_t *__restrict__ lo, const int32_t *__restrict__ hi, int B, int T,
                                             int stride, int kind, float *__restrict__ y, int32_t *__restrict__ arg) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)B * F) return;
  const int b = (int)(id / F), f = (int)(id % F);
  int c = 0, l = 0, h = 0;
  if constexpr (!TAB) c = centre[b], l = lo[b], h = hi[b];
  const int32_t *tab = centre + (long)b * T;      // TAB: `centre` is the (B, T) row table
  float acc = kind == TN_POOL_MAX ? -INFINITY : 0.f;
  int at = 0;
  for (int t = 0; t < T; ++t) {
    long row;
    if constexpr (TAB) row = min(max(tab[t], 0), rows - 1);
    else row = window_row(c, l, h, t, T, stride, rows);
    const float v = x[row * F + f];
    if constexpr (ARG) {
      if (v > acc) at = t;
    }
    acc = kind == TN_POOL_MAX ? fmaxf(acc, v) : acc + v;
  }
  y[id] = kind == TN_POOL_MAX ? acc : acc / (float)T;
  if constexpr (ARG) arg[id] = at;
}

template <int G, int NB, bool TAB, bool ARG>
int launch_window_nb(const float *gi, int ldgi, int rows, const float *whT, const float *bh, const int32_t *centre,
                     const int32_t *lo, const int32_t *hi, float *pooled, int B, int T, int stride, int H, int32_t *steps,
                     hipStream_t s) {
  const dim3 grid((B + NB - 1) / NB, 2), block(G * H);
  const size_t lds = (size_t)(NB * H * 2 + NB * G * H) * sizeof(float);
#define TN_WIN_LAUNCH(KR_, DPP_, MT_)                                                                                          \
  hipLaunchKernelGGL((rnn_window_kernel<G, NB, KR_, DPP_, MT_, TAB, ARG>), grid, block, lds, s, gi, ldgi, rows, whT, bh, centre, lo, \
                     hi, pooled, B, T, stride, H, steps)
  if (H == 128) TN_WIN_LAUNCH(128, true, 512);          // the fast route: CNNRNN's width, the weight column in registers
  else if (H % 16 == 0) TN_WIN_LAUNCH(0, true, 1024);
  else if constexpr (ARG && G == 4 && NB == 8) TN_REQUIRE(false, "rnn_window: the plain LSTM form keeps steps at 4 rows per workgroup");
  else TN_WIN_LAUNCH(0, false, 1024);
#undef TN_WIN_LAUNCH
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

}  // namespace

int rnn_window_default_nb(int gates) { return 2 * gates; }

namespace {

template <bool TAB>
int launch_window(int gates, const float *gi, int ldgi, int rows, const float *whT, const float *bh, const int32_t *centre,
                  const int32_t *lo, const int32_t *hi, float *pooled, int B, int T, int stride, int H, int nb, int32_t *steps,
                  hipStream_t s) {
  TN_REQUIRE(gates == 3 || gates == 4, "rnn_window: gates must be 3 or 4");
  TN_REQUIRE(gates * H <= 1024 && H % 4 == 0, "rnn_window: the windowed kernel serves gates*hidden <= 1024 and hidden % 4 == 0");
  TN_REQUIRE(rows > 0 && B > 0 && T > 0 && stride > 0, "rnn_window: bad shape");
  TN_REQUIRE(!TAB || (long)B * T < (1L << 30), "rnn_window: the row table must hold fewer than 2^30 entries");
  if (nb == 0) nb = rnn_window_default_nb(gates);
  if ((size_t)nb * (2 + gates) * H * sizeof(float) > 64 * 1024) nb = 4;      // (the LDS a workgroup may ask for without an attribute)
  // the plain LSTM form at 8 rows is at its 128 registers without the steps: with them it would spill, so it runs 4 rows per
  // workgroup (one unit per thread instead of two); the result does not depend on the rows per workgroup
  if (steps && gates == 4 && nb == 8 && H % 16 != 0) nb = 4;
#define TN_WIN_ARGS gi, ldgi, rows, whT, bh, centre, lo, hi, pooled, B, T, stride, H, steps, s
#define TN_WIN_NB(G_, NB_)                                                                    \
  if (gates == G_ && nb == NB_)                                                               \
    return steps ? launch_window_nb<G_, NB_, TAB, true>(TN_WIN_ARGS) : launch_window_nb<G_, NB_, TAB, false>(TN_WIN_ARGS)
  TN_WIN_NB(3, 4);
  TN_WIN_NB(3, 6);
  TN_WIN_NB(4, 4);
  TN_WIN_NB(4, 8);
#undef TN_WIN_NB
#undef TN_WIN_ARGS
  TN_REQUIRE(false, "rnn_window: rows per workgroup must be 4 or 6 (GRU) / 4 or 8 (LSTM)");
}

template <bool TAB>
int launch_pool(const float *x, int rows, int F, const int32_t *centre, const int32_t *lo, const int32_t *hi, int B, int T,
                int stride, int kind, float *y, int32_t *arg, hipStream_t s) {
  const long total = (long)B * F;
  TN_REQUIRE(!arg || kind == TN_POOL_MAX, "temporal_pool_windows: the step of a maximum exists for the max pool only");
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (arg) hipLaunchKernelGGL((temporal_pool_windows_kernel<TAB, true>), grid, block, 0, s, x, rows, F, centre, lo, hi, B, T, stride, kind, y, arg);
  else hipLaunchKernelGGL((temporal_pool_windows_kernel<TAB, false>), grid, block, 0, s, x, rows, F, centre, lo, hi, B, T, stride, kind, y, arg);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

}  // namespace

int launch_rnn_window(int gates, const float *gi, int ldgi, int rows, const float *whT, const float *bh, const int32_t *centre,
                      const int32_t *lo, const int32_t *hi, float *pooled, int B, int T, int stride, int H, int nb,
                      hipStream_t s, int32_t *steps) {
  return launch_window<false>(gates, gi, ldgi, rows, whT, bh, centre, lo, hi, pooled, B, T, stride, H, nb, steps, s);
}

int launch_rnn_window_rows(int gates, const float *gi, int ldgi, int rows, const float *whT, const float *bh, const int32_t *idx,
                           float *pooled, int B, int T, int H, int nb, hipStream_t s, int32_t *steps) {
  return launch_window<true>(gates, gi, ldgi, rows, whT, bh, idx, nullptr, nullptr, pooled, B, T, 1, H, nb, steps, s);
}

int launch_temporal_pool_windows(const float *x, int rows, int F, const int32_t *centre, const int32_t *lo, const int32_t *hi,
                                 int B, int T, int stride, int kind, float *y, hipStream_t s, int32_t *arg) {
  return launch_pool<false>(x, rows, F, centre, lo, hi, B, T, stride, kind, y, arg, s);
}

int launch_temporal_pool_rows(const float *x, int rows, int F, const int32_t *idx, int B, int T, int kind, float *y,
                              hipStream_t s, int32_t *arg) {
  return launch_pool<true>(x, rows, F, idx, nullptr, nullptr, B, T, 1, kind, y, arg, s);
}
