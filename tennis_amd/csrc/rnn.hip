// K9/K10/K11 — gluon.rnn.GRU / LSTM (layout 'NTC', optionally bidirectional)
// and the temporal max/mean that follows it (reference
// models/vision/definitions.py:94-96,106-107 and 66-69; one bidirectional layer
// of GNMTEncoder, models/captioning/gnmt.py:141-148).  fp32 throughout so the
// sequential recurrence stays within 1e-3 of the CPU oracle.
//
//   (a) one big i2h GEMM over all B*T rows and both directions (linear.hip);
//   (b) a persistent recurrent kernel: one workgroup per (direction, group of
//       NB batch rows) walks all T steps without leaving the device.  Thread j
//       owns gate row j: it streams column j of the k-major h2h matrix
//       (L2-resident, coalesced across threads) against h held in LDS, the
//       gate pre-activations meet in LDS and the same workgroup applies the
//       gate non-linearities.  valid_length semantics of
//       BidirectionalCell.unroll(valid_length=...) [EXT]: steps >= valid_len
//       do not update state and emit zeros; the reverse pass starts at
//       valid_len-1.  Past G*H = 1024 gate rows (up to 2048: LSTM H = 512,
//       GRU H = 680) a thread owns two rows: rnn_recurrent_wide_kernel.
#include "common.h"
#include "linear.h"
#include "rnn.h"
#include "rnn_dot.h"

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// The cell phase of one step for one (batch row, unit u): from the unit's G input pre-activations gq (i2h + b_i2h) and the row's h2h
// pre-activations q [G*H] (LDS) to the new state in *h (LSTM: and *c), the emitted *out, and - save non-null - the record BPTT reads,
// row srow of [dirs][B*T][(G+1)*H]: GRU r | z | n | (W_hn h + b_hn), LSTM i | f | g | o | c_t.
template <int G>
__device__ __forceinline__ void rnn_cell_forward(const float (&gq)[G], const float *q, int H, int u, float *h, float *c,
                                                 float *__restrict__ save, long srow, float *__restrict__ out) {
#pragma clang fp contract(off)   // the roundings below are the contract: a product is fused where fmaf says so and nowhere else
  float hn;
  if constexpr (G == 3) {
    const float r = sigmoidf_(gq[0] + q[u]);
    const float z = sigmoidf_(gq[1] + q[H + u]);
    const float n = tanhf(fmaf(r, q[2 * H + u], gq[2]));
    hn = fmaf(1.f - z, n, z * *h);
    if (save) {
      float *sv = save + srow * (4 * H);
      sv[u] = r; sv[H + u] = z; sv[2 * H + u] = n; sv[3 * H + u] = q[2 * H + u];
    }
  } else {
    const float ig = sigmoidf_(gq[0] + q[u]);
    const float fg = sigmoidf_(gq[1] + q[H + u]);
    const float gg = tanhf(gq[2] + q[2 * H + u]);
    const float og = sigmoidf_(gq[3] + q[3 * H + u]);
    const float c2 = fmaf(ig, gg, fg * *c);
    *c = c2;
    hn = og * tanhf(c2);
    if (save) {
      float *sv = save + srow * (5 * H);
      sv[u] = ig; sv[H + u] = fg; sv[2 * H + u] = gg; sv[3 * H + u] = og; sv[4 * H + u] = c2;
    }
  }
  *h = hn;
  *out = hn;
}

// One workgroup = one direction x NB batch rows, all T steps; thread j owns gate row j of W_hh.
//   * Per step a CU needs 4*G*H*H bytes of W_hh: at 64 B/clk of L1 fill that stream alone costs as much as the
//     arithmetic, so the first KR k-values of the thread's weight column live in REGISTERS for the whole sequence
//     (KR = H when the block is small enough for a 256-register budget: nothing is re-read), the rest is streamed
//     with 16 loads in flight (batched by hand: the compiler otherwise waits for every group of four).
//   * NB = 4 rows when the batch fills the chip, 1 otherwise: the step is also bound by FMA issue and by the LDS
//     reads of h (both ~ NB*H per thread), so small batches are spread over four times as many CUs.
// The dot product runs over k in ascending order whatever KR and NB are (bit-identical results).
template <int G, int NB, int KR, int MAXT>  // G: 3 = GRU [r,z,n], 4 = LSTM [i,f,g,o]
__global__ __launch_bounds__(MAXT) void rnn_recurrent_kernel(
    const float *__restrict__ gi, int ldgi,  // [B*T][dirs*G*H] i2h + b_i2h
    const float *__restrict__ whT,           // [dirs][H][G*H]
    const float *__restrict__ bh,            // [dirs][G*H]
    const int32_t *__restrict__ valid_len,   // [B] or null
    float *__restrict__ seq, int ldo,        // [B*T][dirs*H]
    float *__restrict__ h_last, float *__restrict__ c_last,  // [dirs][B][H]
    float *__restrict__ save,                // [dirs][B*T][(G+1)*H] or null: what BPTT needs (rnn_bptt.hip)
    int B, int T, int H) {
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

  for (int i = j; i < NB * H; i += GH) {
    hs[i] = 0.f;
    if (G == 4) cs[i] = 0.f;
  }
  __syncthreads();

  for (int s = 0; s < T; ++s) {
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = bj;
    rnn_dot_stream<NB, KR>(acc, wr, wcol, GH, hs, H, H);
#pragma unroll
    for (int b = 0; b < NB; ++b) gh[b * GH + j] = acc[b];
    __syncthreads();
    for (int idx = j; idx < NB * H; idx += GH) {
      const int b = idx / H, u = idx - b * H;
      const int bg = b0 + b;
      if (bg >= B) continue;
      const int vlen = valid_len ? valid_len[bg] : T;
      if (s >= vlen) continue;
      const int ti = dir ? (vlen - 1 - s) : s;
      const float *g = gi + ((long)bg * T + ti) * ldgi + dir * GH;
      float gq[G];
#pragma unroll
      for (int e = 0; e < G; ++e) gq[e] = g[e * H + u];
      rnn_cell_forward<G>(gq, gh + b * GH, H, u, hs + idx, cs + idx, save, (long)dir * B * T + (long)bg * T + ti,
                          seq + ((long)bg * T + ti) * ldo + dir * H + u);
    }
    __syncthreads();
  }
  for (int idx = j; idx < NB * H; idx += GH) {
    const int b = idx / H, u = idx - b * H;
    if (b0 + b >= B) continue;
    if (h_last) h_last[((long)dir * B + b0 + b) * H + u] = hs[idx];
    if (c_last && G == 4) c_last[((long)dir * B + b0 + b) * H + u] = cs[idx];
  }
}

// The same recurrence for the blocks whose weight columns do not fit the registers (G*H > 512: GRU / LSTM with H = 256, the
// captioner's encoder), one batch row per workgroup.  What bounded the kernel above there, per step: the L1 fill of the streamed
// weights (160 of 256 k-values x 768 rows x 4 B = 480 KB at 64 B/clk), the LDS pipe (every lane reading the same h values:
// 64 ds_read_b128 per wave) and the latency of the step's gi loads behind the barrier.  Here
//   * the k-values of a thread's column are split three ways: KR in registers, KL in LDS ([k/4][row][4]: conflict-free 16-byte
//     reads; as much as the 160 KB hold), the rest streamed with 16 loads in flight;
//   * h is not read per FMA: a lane reads 16 bytes per 16 k-values (lane l holds h[k0 + 4 (l mod 4) + e], e = 0..3) and the FMAs
//     take their h operand through DPP quad_perm:[j,j,j,j] (v_fmac_f32_dpp: lane j of the quad, broadcast to the quad) -
//     4 x fewer LDS instructions, no extra VALU work;
//   * the step's gi values are requested before the dot product.
// The dot product still runs over k in ascending order with one accumulator: results are bit-identical to the kernel above.
template <int G, int KR, int KL, int MAXT>
__global__ __launch_bounds__(MAXT) void rnn_recurrent_big_kernel(
    const float *__restrict__ gi, int ldgi, const float *__restrict__ whT, const float *__restrict__ bh,
    const int32_t *__restrict__ valid_len, float *__restrict__ seq, int ldo, float *__restrict__ h_last,
    float *__restrict__ c_last, float *__restrict__ save, int B, int T, int H) {
  static_assert(KR % 16 == 0 && KL % 16 == 0, "whole 16-wide h chunks");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int GH = G * H;
  float *hs = lds;                 // [H]
  float *gh = hs + H;              // [GH]
  float *cs = gh + GH;             // [H] (LSTM)
  float *wl = cs + H;              // [KL/4][GH][4]
  const int j = threadIdx.x, lane4 = (j & 3) * 4;
  const int dir = blockIdx.y, bg = blockIdx.x;
  const float *wcol = whT + (long)dir * H * GH + j;
  const float bj = bh[dir * GH + j];
  float wr[KR];
#pragma unroll
  for (int k = 0; k < KR; ++k) wr[k] = wcol[(long)k * GH];
  rnn_dot_fill_lds<KR, KL>(wl, GH, j, wcol, GH);
  if (j < H) {
    hs[j] = 0.f;
    if (G == 4) cs[j] = 0.f;
  }
  const int vlen = valid_len ? valid_len[bg] : T;
  __syncthreads();

  for (int s = 0; s < T; ++s) {
    // this step's input pre-activations of the units the thread finishes below (requested now, used after the barrier)
    const bool live = j < H && s < vlen;
    const int ti = dir ? (vlen - 1 - s) : s;
    float gq[G];
    if (live) {
      const float *g = gi + ((long)bg * T + ti) * ldgi + dir * GH;
#pragma unroll
      for (int e = 0; e < G; ++e) gq[e] = g[e * H + j];
    }
    const float acc = rnn_dot_big<KR, KL>(bj, wr, wl, GH, j, wcol, GH, hs, H, lane4);
    gh[j] = acc;
    __syncthreads();
    if (live)
      rnn_cell_forward<G>(gq, gh, H, j, hs + j, cs + j, save, (long)dir * B * T + (long)bg * T + ti,
                          seq + ((long)bg * T + ti) * ldo + dir * H + j);
    __syncthreads();
  }
  if (j < H) {
    if (h_last) h_last[((long)dir * B + bg) * H + j] = hs[j];
    if (c_last && G == 4) c_last[((long)dir * B + bg) * H + j] = cs[j];
  }
}

// The same recurrence for 1024 < G*H <= 2048 (LSTM up to H = 512, GRU up to H = 680), where a workgroup has fewer threads than gate
// rows: a thread owns TWO rows, j and j + blockDim.x (rnn.h rnn_wide_route: the block is half the rows, in whole waves).  A row past
// G*H reads the last column and stores nothing, so the loops carry no branch.  Both columns are streamed with 16 k-values in flight
// each; the float4 of h read from LDS serves both rows.  Nothing of W_hh stays in registers or LDS: per step a workgroup streams all
// 4*G*H*H bytes (3 MB at GRU H = 512, 4 MB at LSTM H = 512) from L2 / Infinity Cache, and that stream bounds the step.
// Per row the dot product is that of rnn_recurrent_kernel - one accumulator, the bias first, k ascending - and the cell phase is its
// loop with the block size as stride: results are bit-identical wherever both kernels can run.
template <int G, int NB>
__global__ __launch_bounds__(1024) void rnn_recurrent_wide_kernel(
    const float *__restrict__ gi, int ldgi, const float *__restrict__ whT, const float *__restrict__ bh,
    const int32_t *__restrict__ valid_len, float *__restrict__ seq, int ldo, float *__restrict__ h_last,
    float *__restrict__ c_last, float *__restrict__ save, int B, int T, int H) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int GH = G * H, nt = blockDim.x;
  float *hs = lds;                 // [NB][H]
  float *gh = hs + NB * H;         // [NB][GH]
  float *cs = gh + NB * GH;        // [NB][H] (LSTM)
  const int j = threadIdx.x;
  const int dir = blockIdx.y;
  const int b0 = blockIdx.x * NB;
  const int row[2] = {j, j + nt};                                 // gate rows
  const bool own[2] = {row[0] < GH, row[1] < GH};
  const float *wcol[2];
  float bj[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int rr = min(row[r], GH - 1);
    wcol[r] = whT + (long)dir * H * GH + rr;
    bj[r] = bh[dir * GH + rr];
  }

  for (int i = j; i < NB * H; i += nt) {
    hs[i] = 0.f;
    if (G == 4) cs[i] = 0.f;
  }
  __syncthreads();

  for (int s = 0; s < T; ++s) {
    float acc[2][NB];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[r][b] = bj[r];
    rnn_dot_stream2_shared<NB>(acc, wcol, GH, hs, H, H);
#pragma unroll
    for (int r = 0; r < 2; ++r)
      if (own[r]) {
#pragma unroll
        for (int b = 0; b < NB; ++b) gh[b * GH + row[r]] = acc[r][b];
      }
    __syncthreads();
    for (int idx = j; idx < NB * H; idx += nt) {
      const int b = idx / H, u = idx - b * H;
      const int bg = b0 + b;
      if (bg >= B) continue;
      const int vlen = valid_len ? valid_len[bg] : T;
      if (s >= vlen) continue;
      const int ti = dir ? (vlen - 1 - s) : s;
      const float *g = gi + ((long)bg * T + ti) * ldgi + dir * GH;
      float gq[G];
#pragma unroll
      for (int e = 0; e < G; ++e) gq[e] = g[e * H + u];
      rnn_cell_forward<G>(gq, gh + b * GH, H, u, hs + idx, cs + idx, save, (long)dir * B * T + (long)bg * T + ti,
                          seq + ((long)bg * T + ti) * ldo + dir * H + u);
    }
    __syncthreads();
  }
  for (int idx = j; idx < NB * H; idx += nt) {
    const int b = idx / H, u = idx - b * H;
    if (b0 + b >= B) continue;
    if (h_last) h_last[((long)dir * B + b0 + b) * H + u] = hs[idx];
    if (c_last && G == 4) c_last[((long)dir * B + b0 + b) * H + u] = cs[idx];
  }
}

__global__ void temporal_pool_kernel(const float *__restrict__ x, int B, int T, int F, int kind,
                                     float *__restrict__ y) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)B * F) return;
  const int b = (int)(id / F), f = (int)(id % F);
  const float *p = x + (long)b * T * F + f;
  float acc = kind == TN_POOL_MAX ? -INFINITY : 0.f;
  for (int t = 0; t < T; ++t) {
    const float v = p[(long)t * F];
    acc = kind == TN_POOL_MAX ? fmaxf(acc, v) : acc + v;
  }
  y[id] = kind == TN_POOL_MAX ? acc : acc / (float)T;
}

__global__ void prf1_kernel(const float *__restrict__ logits, const int32_t *__restrict__ labels, int rows,
                            int classes, unsigned long long *__restrict__ mat) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float *p = logits + (long)r * classes;
  int best = 0;
  float bv = p[0];
  for (int c = 1; c < classes; ++c)
    if (p[c] > bv) { bv = p[c]; best = c; }   // first maximum, like ndarray.argmax
  const int lab = labels[r];
  if (lab >= 0 && lab < classes) atomicAdd(mat + (long)lab * classes + best, 1ULL);
}

}  // namespace

// tn_dbg_rnn_force_wide: a test hook, off unless a test turns it on (process-wide; not synchronised with launches in flight)
static bool g_rnn_force_wide = false;
void rnn_set_force_wide(bool on) { g_rnn_force_wide = on; }
bool rnn_takes_wide(int gates, int H) { return gates * H > 1024 || g_rnn_force_wide; }
static std::atomic<long> g_rnn_wide_launches{0};
void rnn_count_wide_launch() { g_rnn_wide_launches.fetch_add(1, std::memory_order_relaxed); }
long rnn_wide_launches() { return g_rnn_wide_launches.load(std::memory_order_relaxed); }

template <int G>
static int rnn_recurrent_launch(const float *gi, int ldgi, const float *whT, const float *bh, const int32_t *valid_len, float *seq,
                                int ldo, float *h_last, float *c_last, int B, int T, int H, int dirs, hipStream_t s, float *save) {
#define TN_RNN_LAUNCH(KERNEL, GRID, BLOCK, LDS) \
  hipLaunchKernelGGL((KERNEL), GRID, BLOCK, LDS, s, gi, ldgi, whT, bh, valid_len, seq, ldo, h_last, c_last, save, B, T, H)
  if (rnn_takes_wide(G, H)) {   // two gate rows per thread (rnn.h rnn_wide_route)
    const tn_rnn_wide_route wr = rnn_wide_route(G, B, H, dirs);
    const dim3 wgrid((B + wr.nb - 1) / wr.nb, dirs), wblock(wr.threads);
    // (the forward kernel's LDS stays below the 64 KiB a launch may ask for unraised: 54 KiB at GRU H = 680, four rows)
    if (wr.nb == 4) TN_RNN_LAUNCH((rnn_recurrent_wide_kernel<G, 4>), wgrid, wblock, wr.lds_fwd);
    else TN_RNN_LAUNCH((rnn_recurrent_wide_kernel<G, 1>), wgrid, wblock, wr.lds_fwd);
    rnn_count_wide_launch();
    TN_HIP_CHECK(hipGetLastError());
    return TN_OK;
  }
  const tn_rnn_route route = rnn_route(G, B, H, dirs);   // rows per workgroup / register-resident prefix / big form (rnn.h)
  const dim3 grid((B + route.nb - 1) / route.nb, dirs), block(G * H);
  if (route.big) {   // one row per workgroup and a column that does not fit the registers (H = 256): registers + LDS + stream, h through DPP
    constexpr tn_rnn_big_split sp = rnn_big_split(G);
    TN_SET_ATTR_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void *)rnn_recurrent_big_kernel<G, sp.kr, sp.kl, sp.threads>,
                                                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    TN_RNN_LAUNCH((rnn_recurrent_big_kernel<G, sp.kr, sp.kl, sp.threads>), grid, block, route.lds_fwd);
  }
  // (register-resident weights only with one row per workgroup: with four the unrolled prefix spills)
  else if (route.nb == 4) TN_RNN_LAUNCH((rnn_recurrent_kernel<G, 4, 0, 1024>), grid, block, route.lds_fwd);
  else if (route.kr == 128) TN_RNN_LAUNCH((rnn_recurrent_kernel<G, 1, 128, 512>), grid, block, route.lds_fwd);
  else if (route.kr == 96) TN_RNN_LAUNCH((rnn_recurrent_kernel<G, 1, 96, 768>), grid, block, route.lds_fwd);
  else if (route.kr == 64) TN_RNN_LAUNCH((rnn_recurrent_kernel<G, 1, 64, 1024>), grid, block, route.lds_fwd);
  else TN_RNN_LAUNCH((rnn_recurrent_kernel<G, 1, 0, 1024>), grid, block, route.lds_fwd);
#undef TN_RNN_LAUNCH
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

int launch_rnn_recurrent(int gates, const float *gi, int ldgi, const float *whT, const float *bh,
                         const int32_t *valid_len, float *seq, int ldo, float *h_last, float *c_last, int B, int T,
                         int H, int dirs, hipStream_t s, float *save) {
  TN_REQUIRE(gates == 3 || gates == 4, "rnn: gates must be 3 or 4");
  TN_REQUIRE(H > 0 && gates * H <= 2048 && H % 4 == 0, "rnn: gates*hidden must be <= 2048 and hidden % 4 == 0");
  return gates == 3 ? rnn_recurrent_launch<3>(gi, ldgi, whT, bh, valid_len, seq, ldo, h_last, c_last, B, T, H, dirs, s, save)
                    : rnn_recurrent_launch<4>(gi, ldgi, whT, bh, valid_len, seq, ldo, h_last, c_last, B, T, H, dirs, s, save);
}

int launch_temporal_pool(const float *x, int B, int T, int F, int kind, float *y, hipStream_t s) {
  const long total = (long)B * F;
  hipLaunchKernelGGL(temporal_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, B, T, F, kind,
                     y);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

int launch_prf1(const float *logits, const int32_t *labels, int rows, int classes, int64_t *mat, hipStream_t s) {
  hipLaunchKernelGGL(prf1_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, logits, labels, rows, classes,
                     (unsigned long long *)mat);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}
