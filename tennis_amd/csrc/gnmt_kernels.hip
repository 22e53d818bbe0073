// The captioner's kernels, fp32 throughout, and their launchers (gnmt_kernels.h): the decode step shared by the beam search and by
// teacher forcing, the search's bookkeeping, the losses and the training step's backward kernels.
// One decode step = four launches: a stacked-gate GEMM per cell (linear.hip), dec_attention_kernel (cell-0 gates + attention) and
// dec_beam_kernel (cell-1 gates + projection + beam update + the next step's gathered inputs) resp. dec_cell_kernel + the
// projection GEMM (teacher forcing, training).
// On request (gnmt.py:302-303,402-403) the steps' attention weights are kept: teacher forcing stores them in place, the beam search
// keeps every step's rows in a history and gathers the final hypotheses' rows along their back-pointers (beam_att_rows_kernel,
// beam_att_gather_kernel).
#include <cmath>
#include <cstring>

#include "gnmt_kernels.h"
#include "linear.h"

namespace {

constexpr float kNeg = -1e18f;
// element (row r, column k) of a decoder cell's step-input matrix: row-major with pitch ld > 0, or k-group-major
// ([k/4][rows][4], the operand form of lat_tile_f32<.., true>) with -ld rows
__device__ __forceinline__ long xidx(long r, int k, int ld) { return ld > 0 ? r * ld + k : ((long)(k >> 2) * (-ld) + r) * 4 + (k & 3); }

__device__ __forceinline__ float sigm(float v) { return 1.0f / (1.0f + expf(-v)); }
// The cells' gate arithmetic on the four stacked pre-activations of a unit - GRU [r, z, n_i2h, n_h2h] (r and z already summed over
// both branches), LSTM [i, f, g, o]: the activations, and the new state from them and the previous one.  dec_cell_kernel and the
// two backward kernels go through these; dec_attention_kernel and dec_beam_kernel spell the same lines out in place, because
// calling the functions there changes the two kernels' instruction schedule (compared on the assembly) and they are the hot ones.
struct GruGates { float r, z, n; };
struct LstmGates { float i, f, g, o; };
__device__ __forceinline__ GruGates gru_gates(float ga, float gb, float gc, float gd) {
  const float rg = sigm(ga), zg = sigm(gb);
  return {rg, zg, tanhf(gc + rg * gd)};
}
__device__ __forceinline__ LstmGates lstm_gates(float ga, float gb, float gc, float gd) { return {sigm(ga), sigm(gb), tanhf(gc), sigm(gd)}; }
__device__ __forceinline__ float gru_cell(float ga, float gb, float gc, float gd, float hprev) {
  const GruGates a = gru_gates(ga, gb, gc, gd);
  return (1.f - a.z) * a.n + a.z * hprev;
}
__device__ __forceinline__ float lstm_cell(float ga, float gb, float gc, float gd, float cprev, float &c) {    // returns h, c = the new cell state
  const LstmGates a = lstm_gates(ga, gb, gc, gd);
  // f * c_prev + i * g with the rounding the cell kernels have always had (f * c_prev rounded, i * g fused into the sum), spelled
  // out because the compiler is free to fuse either product and picks by context
  c = fmaf(a.i, a.g, a.f * cprev);
  return a.o * tanhf(c);
}

// Wave-wide maximum / sum in six DPP stages (row shifts + row broadcasts, result in lane 63, handed to every lane through an SGPR)
__device__ __forceinline__ float wave_max(float v) {
  float m = v;
#define TN_DPP_F(ctrl, rmask) m = fmaxf(m, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(m), __float_as_int(m), ctrl, rmask, 0xf, false)));
  TN_DPP_F(0x111, 0xf) TN_DPP_F(0x112, 0xf) TN_DPP_F(0x114, 0xf) TN_DPP_F(0x118, 0xf) TN_DPP_F(0x142, 0xa) TN_DPP_F(0x143, 0xc)
#undef TN_DPP_F
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 63));
}
__device__ __forceinline__ float wave_sum(float v) {
  float m = v;
#define TN_DPP_F(ctrl, rmask) m += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), ctrl, rmask, 0xf, false));
  TN_DPP_F(0x111, 0xf) TN_DPP_F(0x112, 0xf) TN_DPP_F(0x114, 0xf) TN_DPP_F(0x118, 0xf) TN_DPP_F(0x142, 0xa) TN_DPP_F(0x143, 0xc)
#undef TN_DPP_F
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 63));
}

// ---- beam-search step kernels: 1024 threads = 16 waves (kBeamThreads, step_groups: gnmt_kernels.h) ----
#ifdef TN_DEC_STAMPS  // tuning builds only (EXTRA=-DTN_DEC_STAMPS): phase boundaries of workgroup 0, 100 MHz ticks
__device__ long long g_dec_stamps[24];
#define DEC_STAMP(i) do { __syncthreads(); if (blockIdx.x == 0 && threadIdx.x == 0) g_dec_stamps[i] = wall_clock64(); } while (0)
#else
#define DEC_STAMP(i)
#endif
// Beam-search step, first launch, one workgroup (16 waves) per decoder row (the step is latency-bound - few workgroups,
// dependent L2 round trips - so it pays to spread the rows over CUs even though the beams of a clip each re-read the clip's key
// projection and memory from L2):
//   first decoder cell's gate arithmetic on the stacked pre-activations g0 (R,4H) — GRU columns
//   [r, z, n_i2h, n_h2h] (r and z already summed over both branches), LSTM [i, f, g, o]; h_prev = last H columns
//   of the step input x0 — the new state goes to hn (R,H) (+ cn) and to x1[:, 0:H];
//   scaled-Luong scores against the TRANSPOSED key projection kpT (B,H,Tp) (Tp = T rounded up to 4), masked softmax (one
//   wave), context from mem (B,T,H) -> ctx (R,H) and x1[:, H:2H].
__global__ __launch_bounds__(kBeamThreads) void dec_attention_kernel(
    const float *__restrict__ g0, const float *__restrict__ hprev, int ldh, const float *__restrict__ cprev, int lstm,
    float *__restrict__ hn, float *__restrict__ cn, float *__restrict__ x1, int ldx1,
    const float *__restrict__ kpT, const float *__restrict__ mem, const int32_t *__restrict__ valid_len,
    float *__restrict__ ctx, int beam, int rows, int T, int H, float *__restrict__ wsave = nullptr,
    const int32_t *__restrict__ tok = nullptr, const int32_t *__restrict__ par = nullptr, const float *__restrict__ ew = nullptr,
    const float *__restrict__ p0 = nullptr, int split = 16, long wpitch = 0) {
  // wsave != NULL: the row's T attention weights are stored at wsave + row * wpitch (wpitch 0: T, rows back to back)
  // ew != NULL (beam search, two decoder layers, from the second step on): the row's pre-activations are put together here,
  // g = ew[tok[row]] + p0[parent row] (dec_beam_kernel), and h_prev / c_prev are the PARENT row's (hprev / cprev then hold
  // the previous step's new states, one row per beam, pitch ldh / H)
  extern __shared__ float sm[];   // q[H] | w[Tp] | part[16 * max(Tp, H)]
  const int Tp = (T + 3) & ~3;
  float *q = sm, *w = q + H, *part = w + Tp;
  // workgroup -> decoder row: workgroups go to the 8 XCDs round robin, and the `beam` rows of a clip read the same key projection
  // and memory (2 T H floats): rows of one clip are given to workgroups of one XCD, so that a clip's data sits in one L2
  // (4 MB each) instead of `beam` of them
  long r = blockIdx.x;
  {
    const int nclips = (int)gridDim.x / beam, full = (nclips / 8) * 8 * beam, id = blockIdx.x;
    if (id < full) {
      const int slot = id >> 3;
      r = (long)((id & 7) + 8 * (slot / beam)) * beam + slot % beam;
    }
  }
  const int b = (int)(r / beam), t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int vl = min(max(valid_len[b], 0), T);
  const float inv = 1.0f / sqrtf((float)H);
  DEC_STAMP(0);
  // ---- cell 0 ----
  for (int u = t; u < H; u += kBeamThreads) {
    const long rp = ew ? (long)b * beam + par[r] : r;
    float ga, gb, gc, gd;
    if (ew) {
      const int word = tok[r];
      const float *e = ew + (long)(word > 0 ? word : 0) * 4 * H, *q0 = p0 + rp * 4 * H;
      ga = e[u] + q0[u]; gb = e[H + u] + q0[H + u]; gc = e[2 * H + u] + q0[2 * H + u]; gd = e[3 * H + u] + q0[3 * H + u];
    } else {
      const float *g = g0 + r * 4 * H;
      ga = g[u]; gb = g[H + u]; gc = g[2 * H + u]; gd = g[3 * H + u];
    }
    float v;
    if (lstm) {      // (lstm_cell / gru_cell in place, see there)
      const float ig = sigm(ga), fg = sigm(gb), gg = tanhf(gc), og = sigm(gd);
      const float c2 = fg * cprev[rp * H + u] + ig * gg;
      cn[r * H + u] = c2;
      v = og * tanhf(c2);
    } else {
      const float rg = sigm(ga), zg = sigm(gb);
      const float ng = tanhf(gc + rg * gd);
      v = (1.f - zg) * ng + zg * hprev[rp * ldh + u];
    }
    hn[r * H + u] = v;
    x1[xidx(r, u, ldx1)] = v;
    q[u] = v * inv;
  }
  __syncthreads();
  DEC_STAMP(1);
  // ---- scores: thread = (slice of H, four source steps); HG partial sums per step ----
  // (the groups follow the PADDED length, as att_lds_bytes counts the partial rows: dealing a clip shorter than T over fewer
  // threads would ask for more rows of pitch Tp than the launch has LDS for, once T > 256)
  const int S4 = (vl + 3) >> 2, CG = step_groups(Tp >> 2, split), HG = kBeamThreads / CG;
  {
    const int hg = t / CG, hn_ = (H + HG - 1) / HG, h0 = hg * hn_, h1 = min(H, h0 + hn_);
    const float *kp = kpT + (long)b * H * Tp;
    for (int s4 = t % CG; s4 < S4; s4 += CG) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      int h = h0;
      for (; h + 16 <= h1; h += 16) {           // 16 x 16 bytes in flight
        float4 kv[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) kv[i] = *(const float4 *)(kp + (long)(h + i) * Tp + 4 * s4);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float qv = q[h + i];
          acc.x = fmaf(kv[i].x, qv, acc.x); acc.y = fmaf(kv[i].y, qv, acc.y); acc.z = fmaf(kv[i].z, qv, acc.z); acc.w = fmaf(kv[i].w, qv, acc.w);
        }
      }
      for (; h < h1; ++h) {
        const float4 kv = *(const float4 *)(kp + (long)h * Tp + 4 * s4);
        const float qv = q[h];
        acc.x = fmaf(kv.x, qv, acc.x); acc.y = fmaf(kv.y, qv, acc.y); acc.z = fmaf(kv.z, qv, acc.z); acc.w = fmaf(kv.w, qv, acc.w);
      }
      *(float4 *)(part + hg * Tp + 4 * s4) = acc;
    }
  }
  __syncthreads();
  DEC_STAMP(2);
  // ---- the HG partial sums of every step (all threads), then the masked softmax in one wave (masked -> -1e18, weights * mask) ----
  for (int s = t; s < T; s += kBeamThreads) {
    float a = kNeg;
    if (s < vl) {
      a = part[s];
      for (int g = 1; g < HG; ++g) a += part[g * Tp + s];
    }
    w[s] = a;
  }
  __syncthreads();
  if (wid == 0) {
    float mx = -INFINITY;
    for (int s = lane; s < T; s += 64) mx = fmaxf(mx, w[s]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int s = lane; s < T; s += 64) {
      const float e = expf(w[s] - mx);
      w[s] = e;
      sum += e;
    }
    sum = wave_sum(sum);
    const float rs = 1.0f / sum;
    for (int s = lane; s < T; s += 64) {
      const float v = s < vl ? w[s] * rs : 0.f;
      w[s] = v;
      if (wsave) wsave[r * (wpitch ? wpitch : (long)T) + s] = v;      // training / the attention outputs keep the weights
    }
  }
  __syncthreads();
  DEC_STAMP(3);
  // ---- context: thread = (slice of the valid steps, four units); SG partial sums per unit; weights beyond valid_len are 0 ----
  const int U4 = H >> 2, CG2 = step_groups(U4, split), SG = kBeamThreads / CG2;
  {
    const int sg = t / CG2, sn = (vl + SG - 1) / SG, s0 = sg * sn, s1 = min(vl, s0 + sn);
    const float *mv = mem + (long)b * T * H;
    for (int u4 = t % CG2; u4 < U4; u4 += CG2) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      int s = s0;
      for (; s + 16 <= s1; s += 16) {
        float4 m[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) m[i] = *(const float4 *)(mv + (long)(s + i) * H + 4 * u4);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float wv = w[s + i];
          acc.x = fmaf(wv, m[i].x, acc.x); acc.y = fmaf(wv, m[i].y, acc.y); acc.z = fmaf(wv, m[i].z, acc.z); acc.w = fmaf(wv, m[i].w, acc.w);
        }
      }
      if (s < s1) {                              // the rest of the slice, still all in flight at once
        float4 m[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) m[i] = s + i < s1 ? *(const float4 *)(mv + (long)(s + i) * H + 4 * u4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float wv = s + i < s1 ? w[s + i] : 0.f;
          acc.x = fmaf(wv, m[i].x, acc.x); acc.y = fmaf(wv, m[i].y, acc.y); acc.z = fmaf(wv, m[i].z, acc.z); acc.w = fmaf(wv, m[i].w, acc.w);
        }
      }
      *(float4 *)(part + sg * H + 4 * u4) = acc;
    }
  }
  __syncthreads();
  for (int u = t; u < H; u += kBeamThreads) {
    float a = part[u];
    for (int g = 1; g < SG; ++g) a += part[g * H + u];
    ctx[r * H + u] = a;
    x1[xidx(r, H + u, ldx1)] = a;
  }
  DEC_STAMP(4);
}

// (B,T,H) -> (B,H,Tp), Tp = T rounded up to 4: the key projection as the attention kernel reads it (16-byte loads along T)
__global__ void transpose_bth_kernel(const float *__restrict__ src, float *__restrict__ dst, int T, int H) {
  __shared__ float tile[32][33];
  const int Tp = (T + 3) & ~3;
  const int b = blockIdx.z, t0 = blockIdx.y * 32, h0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) tile[i][tx] = (t0 + i < T && h0 + tx < H) ? src[((long)b * T + t0 + i) * H + h0 + tx] : 0.f;
  __syncthreads();
  for (int i = ty; i < 32; i += 8)
    if (h0 + i < H && t0 + tx < Tp) dst[((long)b * H + h0 + i) * Tp + t0 + tx] = tile[tx][i];
}

// Wave-wide best of per-lane (value, index) pairs - value descending, then index ascending - in two DPP reductions of one
// instruction per stage (row shifts + row broadcasts, result in lane 63): the maximum value, then the minimum index among the
// lanes that hold it.  A lane without a candidate passes (-inf, 0xffffffff).
__device__ __forceinline__ void wave_best(float v, unsigned ix, float &wv, unsigned &wi) {
  float m = v;
#define TN_DPP_F(ctrl, rmask) m = fmaxf(m, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(m), __float_as_int(m), ctrl, rmask, 0xf, false)));
  TN_DPP_F(0x111, 0xf) TN_DPP_F(0x112, 0xf) TN_DPP_F(0x114, 0xf) TN_DPP_F(0x118, 0xf)   // row_shr:1,2,4,8 -> lane 15 of a row
  TN_DPP_F(0x142, 0xa) TN_DPP_F(0x143, 0xc)                                             // row_bcast:15 / :31 -> lane 63
#undef TN_DPP_F
  wv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 63));
  unsigned c = v == wv ? ix : 0xffffffffu;
#define TN_DPP_U(ctrl, rmask) c = min(c, (unsigned)__builtin_amdgcn_update_dpp((int)c, (int)c, ctrl, rmask, 0xf, false));
  TN_DPP_U(0x111, 0xf) TN_DPP_U(0x112, 0xf) TN_DPP_U(0x114, 0xf) TN_DPP_U(0x118, 0xf)
  TN_DPP_U(0x142, 0xa) TN_DPP_U(0x143, 0xc)
#undef TN_DPP_U
  wi = (unsigned)__builtin_amdgcn_readlane((int)c, 63);
}

// The `count` largest of n <= 256 elements held four per lane in registers (x[i], index xi[i]; -inf / 0xffffffff where the lane
// has none), descending, ties -> lowest index: one wave, no barrier, nothing re-read.  A round is wave_best plus, in the
// winning lane only, dropping the element.  out_val / out_idx (LDS) receive the winners.
__device__ __forceinline__ void wave_topk_regs(float (&x)[4], unsigned (&xi)[4], int count, float *out_val, int *out_idx) {
  float bv;
  unsigned bix;
  int bpos;
  auto scan = [&]() {
    bv = -INFINITY; bix = 0xffffffffu; bpos = -1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool better = (x[i] > bv) | ((x[i] == bv) & (xi[i] < bix));     // (no short circuit: straight-line selects)
      bv = better ? x[i] : bv; bix = better ? xi[i] : bix; bpos = better ? i : bpos;
    }
  };
  scan();
  for (int k = 0; k < count; ++k) {
    float wv;
    unsigned wi;
    wave_best(bv, bix, wv, wi);
    const bool won = (bpos >= 0) & (bix == wi) & (bv == wv);       // this lane owned the winner: record, drop it, look again
    if (won) {
      out_idx[k] = (int)wi;
      out_val[k] = wv;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool drop = won & (i == bpos);
      x[i] = drop ? -INFINITY : x[i];
      xi[i] = drop ? 0xffffffffu : xi[i];
    }
    scan();
  }
}
// The same over arr[0..n) in LDS for any n, element p has index idx[p] (idx != NULL) or base + p: a lane owns the elements
// p = lane mod 64 and rescans them when it has won (the dropped element becomes -inf in LDS).
__device__ __forceinline__ void wave_topk(float *arr, const int *idx, int base, int n, int count, float *out_val, int *out_idx, int lane) {
  if (n <= 256) {
    float x[4];
    unsigned xi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = lane + 64 * i;
      x[i] = p < n ? arr[p] : -INFINITY;
      xi[i] = p < n ? (unsigned)(idx ? idx[p] : base + p) : 0xffffffffu;
    }
    wave_topk_regs(x, xi, count, out_val, out_idx);
    return;
  }
  float bv;
  unsigned bix;
  int bpos;
  auto scan = [&]() {
    bv = -INFINITY; bix = 0xffffffffu; bpos = -1;
    for (int p = lane; p < n; p += 64) {
      const float v = arr[p];
      const unsigned ix = (unsigned)(idx ? idx[p] : base + p);
      if (v > bv || (v == bv && ix < bix)) { bv = v; bix = ix; bpos = p; }
    }
  };
  scan();
  for (int k = 0; k < count; ++k) {
    float wv;
    unsigned wi;
    wave_best(bv, bix, wv, wi);
    if (bpos >= 0 && bix == wi && bv == wv) {
      out_idx[k] = (int)wi;
      out_val[k] = wv;
      arr[bpos] = -INFINITY;
      scan();
    }
  }
}

// Beam-search step, last launch, one workgroup per source clip:
//   last decoder cell's gates on g1 (R rows of ldg floats, the first 4H of a row; column layout as in dec_attention_kernel;
//   h_prev / c_prev are the clip's rows of x1[:, 2H:3H] / c1cur) -> projection to the vocabulary (Wp^T streamed once for all
//   beams, 4 partial sums over K) -> per beam row, inside one wave: logits, log-sum-exp, length-penalised candidates and the
//   row's `beam` best -> top-`beam` over [the rows' bests | finished] (the same order as a top-`beam` over [beam*V | finished]:
//   value descending, ties to the lowest index) -> bookkeeping, the step's (parent, word) back-pointers (the token prefixes are
//   rebuilt once at the end, beam_samples_kernel) -> the NEXT step's inputs, re-gathered by parent beam.  Two forms:
//     tok_out == NULL: x0 = [embed(word), ctx[parent], h0[parent]], c0cur; the first cell's gate GEMM is the next step's first launch;
//     tok_out != NULL (two decoder layers): the first cell's pre-activations are linear in x0 and the next step's attention
//       kernel puts them together itself, g0 = ew[word] + p0[parent] with ew = embed . W0[:, 0:E]^T (V,4H; once per model) and
//       p0 = [h0, ctx] . W0[:, E:]^T + b0.  p0 only needs what the attention kernel left in x1, so it is computed by EXTRA
//       workgroups of this launch (blockIdx >= nclips, four 16 x 16 tiles each, lat_tile_f32) on the CUs the clips do not use:
//       3 launches per step, and the gate GEMM on the critical path stays the last cell's.  This kernel then only hands on
//       the words and the parents.
//   Always: x1[:, 2H:3H] = h1[parent], c1cur (LSTM).
struct LatGemmArgs {
  const float *X, *W, *bias;
  float *Y;
  int ldx, ldw, ldy, M, N, K;
};
template <int NBM>
__global__ __launch_bounds__(kBeamThreads) void dec_beam_kernel(
    const float *__restrict__ g1, int ldg, float *__restrict__ x1, int K1, int lstm, float *__restrict__ c1cur,
    const float *__restrict__ wpT, const float *__restrict__ bp, const float *__restrict__ h0n,
    const float *__restrict__ ctx, const float *__restrict__ c0n, float *__restrict__ x0, float *__restrict__ c0cur,
    const float *__restrict__ emb, int H, int E, int V, int beam, int step, float lp, float prev_lp, int eos,
    float *__restrict__ scores, int32_t *__restrict__ alive, int32_t *__restrict__ vlen,
    int32_t *__restrict__ bp_par, int32_t *__restrict__ bp_word, int R, int32_t *__restrict__ any_alive,
    float *__restrict__ hstate, int32_t *__restrict__ parent_out, int32_t *__restrict__ tok_out, int nclips, LatGemmArgs gm, int split) {
  // hstate != NULL: use_residual (gnmt.py:394-395) - the projection sees h + the cell's input x1[:, 0:H], the recurrent
  // state stays h and goes through this (R,H) scratch; parent_out: the chosen parent beam of every row, for the states of
  // the decoder layers between the first and the last one (num_layers > 2)
  extern __shared__ float sm[];   // h1n[H][NP] | c1n[H][NP] | logits[beam*Vp] (the candidates in place) | part[KQ*beam*Vp]
  const int b = blockIdx.x, t = threadIdx.x, K0 = E + 2 * H;     // (K1: pitch of x1 = [input of the last cell (2H) | h_prev])
  constexpr int NP = (NBM + 3) & ~3;   // LDS pitch of one k: NBM beam rows padded to 16-byte multiples
  float *h1n = sm, *c1n = h1n + NP * H, *logits = c1n + NP * H, *part = logits + beam * ((V + 3) & ~3);
  __shared__ float sel_val[16], o_score[16], m_val[16 * 16 + 16];
  __shared__ int sel_idx[16], sel_par[16], sel_word[16], o_alive[16], o_vlen[16], m_idx[16 * 16 + 16];
  const int lane = t & 63, wid = t >> 6;
  if (b >= nclips) {      // p0 tiles for the next step (see above); no output that this launch's clips read
    const int tile = (b - nclips) * 4 + (wid >> 2), ntn = gm.N / 16;
    if (gm.ldx < 0)
      lat_tile_f32<false, true>(gm.X, -4 * gm.ldx, gm.W, gm.ldw, gm.bias, gm.Y, gm.ldy, gm.M, gm.N, gm.K, (tile / ntn) * 16, (tile % ntn) * 16, wid & 3,
                                lane, (float (*)[64][4])(sm + (wid >> 2) * (4 * 64 * 4)));
    else
      lat_tile_f32(gm.X, gm.ldx, gm.W, gm.ldw, gm.bias, gm.Y, gm.ldy, gm.M, gm.N, gm.K, (tile / ntn) * 16, (tile % ntn) * 16, wid & 3, lane,
                   (float (*)[64][4])(sm + (wid >> 2) * (4 * 64 * 4)));
    return;
  }
  // the old state of the beam row this wave will own (loaded now, used after the projection)
  const int rowk = wid < beam ? wid : 0;
  const int al = alive[b * beam + rowk], ovl = vlen[b * beam + rowk];
  const float osc = scores[b * beam + rowk];
  DEC_STAMP(8);
  // ---- cell 1 ----
  for (int idx = t; idx < NBM * H; idx += kBeamThreads) {
    const int k = idx / H, u = idx - k * H;
    float v = 0.f, c2 = 0.f;
    if (k < beam) {
      const long r = (long)b * beam + k;
      const float *g = g1 + r * ldg;
      if (lstm) {      // (lstm_cell / gru_cell in place, see there)
        const float ig = sigm(g[u]), fg = sigm(g[H + u]), gg = tanhf(g[2 * H + u]), og = sigm(g[3 * H + u]);
        c2 = fg * c1cur[r * H + u] + ig * gg;
        v = og * tanhf(c2);
      } else {
        const float rg = sigm(g[u]), zg = sigm(g[H + u]);
        const float ng = tanhf(g[2 * H + u] + rg * g[3 * H + u]);
        v = (1.f - zg) * ng + zg * x1[xidx(r, 2 * H + u, K1)];
      }
      if (hstate) {
        hstate[r * H + u] = v;
        v += x1[xidx(r, u, K1)];
      }
    }
    h1n[u * NP + k] = v;       // k-major: a projection thread reads its NBM rows with one or two wide LDS loads
    c1n[u * NP + k] = c2;
  }
  __syncthreads();
  DEC_STAMP(9);
  // ---- projection: thread = (slice of K, four vocabulary columns), see step_groups; KQ partial sums per logit ----
  const int Vp = (V + 3) & ~3, V4 = Vp >> 2, CGv = step_groups(V4, split), KQ = kBeamThreads / CGv;
  {
    constexpr int NLD = NBM <= 5 ? 16 : NBM <= 8 ? 8 : 2;      // 16-byte loads in flight (registers: NBM float4 sums beside them)
    const int kq = t / CGv, kn = (H + KQ - 1) / KQ, k0 = kq * kn, k1 = min(H, k0 + kn);
    for (int v4 = t % CGv; v4 < V4; v4 += CGv) {
      float4 acc[NBM];
      const float4 bz = kq == 0 ? *(const float4 *)(bp + 4 * v4) : make_float4(0.f, 0.f, 0.f, 0.f);   // (bp padded to Vp)
#pragma unroll
      for (int q = 0; q < NBM; ++q) acc[q] = bz;
      int k = k0;
      for (; k + NLD <= k1; k += NLD) {
        float4 w[NLD];
#pragma unroll
        for (int i = 0; i < NLD; ++i) w[i] = *(const float4 *)(wpT + (long)(k + i) * Vp + 4 * v4);
#pragma unroll
        for (int i = 0; i < NLD; ++i)
#pragma unroll
          for (int q = 0; q < NBM; ++q) {
            const float hv = h1n[(k + i) * NP + q];
            acc[q].x = fmaf(w[i].x, hv, acc[q].x); acc[q].y = fmaf(w[i].y, hv, acc[q].y);
            acc[q].z = fmaf(w[i].z, hv, acc[q].z); acc[q].w = fmaf(w[i].w, hv, acc[q].w);
          }
      }
      for (; k < k1; ++k) {
        const float4 w = *(const float4 *)(wpT + (long)k * Vp + 4 * v4);
#pragma unroll
        for (int q = 0; q < NBM; ++q) {
          const float hv = h1n[k * NP + q];
          acc[q].x = fmaf(w.x, hv, acc[q].x); acc[q].y = fmaf(w.y, hv, acc[q].y);
          acc[q].z = fmaf(w.z, hv, acc[q].z); acc[q].w = fmaf(w.w, hv, acc[q].w);
        }
      }
#pragma unroll
      for (int q = 0; q < NBM; ++q)
        if (q < beam) *(float4 *)(part + (long)(kq * beam + q) * Vp + 4 * v4) = acc[q];
    }
  }
  __syncthreads();
  DEC_STAMP(10);
  // ---- logits = the KQ partial sums (the first one starts from the bias), all threads ----
  for (int c = t; c < beam * V; c += kBeamThreads) {
    const int k = c / V, v = c - k * V;
    float x = part[k * Vp + v];
    for (int g = 1; g < KQ; ++g) x += part[(g * beam + k) * Vp + v];
    logits[k * Vp + v] = x;
  }
  __syncthreads();
  // ---- wave k owns beam row k: log-sum-exp, length-penalised candidates and the row's `beam` best (V <= 256: in registers) ----
  if (wid < beam) {
    const int k = wid;
    float *z = logits + k * Vp;
    if (V <= 256) {
      float x[4];
      unsigned xi[4];
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int v = lane + 64 * i;
        x[i] = v < V ? z[v] : -INFINITY;
        xi[i] = v < V ? (unsigned)(k * V + v) : 0xffffffffu;
        mx = fmaxf(mx, x[i]);
      }
      mx = wave_max(mx);
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < V) sum += expf(x[i] - mx);
      sum = wave_sum(sum);
      const float lse = mx + logf(sum);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < V) x[i] = al ? (osc * prev_lp + (x[i] - lse)) / lp : kNeg;
      wave_topk_regs(x, xi, beam, m_val + k * beam, m_idx + k * beam);
    } else {
      float mx = -INFINITY;
      for (int v = lane; v < V; v += 64) mx = fmaxf(mx, z[v]);
      mx = wave_max(mx);
      float sum = 0.f;
      for (int v = lane; v < V; v += 64) sum += expf(z[v] - mx);
      sum = wave_sum(sum);
      const float lse = mx + logf(sum);
      for (int v = lane; v < V; v += 64) {
        const float logp = z[v] - lse;
        z[v] = al ? (osc * prev_lp + logp) / lp : kNeg;
      }
      wave_topk(z, nullptr, k * V, V, beam, m_val + k * beam, m_idx + k * beam, lane);
    }
    if (lane == 0) {
      o_alive[k] = al; o_vlen[k] = ovl; o_score[k] = osc;
      m_val[beam * beam + k] = al ? kNeg : osc;           // a finished beam competes with its own score
      m_idx[beam * beam + k] = beam * V + k;
    }
  }
  __syncthreads();
  DEC_STAMP(12);
  // ---- top-`beam` of the clip: the rows' bests and the finished beams; the same wave then does the bookkeeping ----
  if (wid == 0) {
    // every candidate counts the candidates that beat it (value, then lower index): the ones beaten by fewer than `beam` are
    // the winners and the count is their place - no dependent rounds.  Up to 64 candidates: one per lane, the others' values
    // come through v_readlane (branch-free); more (beam >= 8): broadcast LDS reads.
    const int n2 = beam * beam + beam;
    if (n2 <= 64) {
      const float v = lane < n2 ? m_val[lane] : -INFINITY;
      const int ix = lane < n2 ? m_idx[lane] : 0x7fffffff;
      int rank = 0;
      for (int j = 0; j < n2; ++j) {
        const float vj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
        const int ij = __builtin_amdgcn_readlane(ix, j);
        rank += (int)(vj > v) | ((int)(vj == v) & (int)(ij < ix));
      }
      if (lane < n2 && rank < beam) { sel_val[rank] = v; sel_idx[rank] = ix; }
    } else {
      for (int p = lane; p < n2; p += 64) {
        const float v = m_val[p];
        const int ix = m_idx[p];
        int rank = 0;
        for (int j = 0; j < n2; ++j) {
          const float vj = m_val[j];
          const int ij = m_idx[j];
          rank += (int)(vj > v) | ((int)(vj == v) & (int)(ij < ix));
        }
        if (rank < beam) { sel_val[rank] = v; sel_idx[rank] = ix; }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  DEC_STAMP(13);
  // ---- bookkeeping ----
  if (t < beam) {
    const int idx = sel_idx[t];
    const bool use_prev = idx >= beam * V;
    const int word = use_prev ? -1 : idx % V;
    const int bid = use_prev ? idx - beam * V : idx / V;
    scores[b * beam + t] = sel_val[t];
    vlen[b * beam + t] = o_vlen[bid] + 1 - (use_prev ? 1 : 0);
    const int al = o_alive[bid] && word != eos;
    alive[b * beam + t] = al;
    sel_par[t] = bid;
    sel_word[t] = word;
    if (parent_out) parent_out[b * beam + t] = bid;
    bp_par[(long)(step - 1) * R + b * beam + t] = bid;
    bp_word[(long)(step - 1) * R + b * beam + t] = word;
    if (al) atomicOr(any_alive, 1);
  }
  __syncthreads();
  DEC_STAMP(14);
  // ---- next step's inputs, states re-gathered by parent beam ----
  if (tok_out) {
    if (t < beam) tok_out[b * beam + t] = sel_word[t];
  } else {
    for (int idx = t; idx < beam * K0; idx += kBeamThreads) {
      const int k = idx / K0, i = idx - k * K0;
      const long r = (long)b * beam + k, pr = (long)b * beam + sel_par[k];
      const int word = sel_word[k];
      float v;
      if (i < E) v = emb[(long)(word > 0 ? word : 0) * E + i];
      else if (i < E + H) v = ctx[pr * H + i - E];
      else v = h0n[pr * H + i - E - H];
      x0[r * K0 + i] = v;
    }
  }
  for (int idx = t; idx < beam * H; idx += kBeamThreads) {
    const int k = idx / H, u = idx - k * H;
    const long r = (long)b * beam + k, pr = (long)b * beam + sel_par[k];
    x1[xidx(r, 2 * H + u, K1)] = hstate ? hstate[pr * H + u] : h1n[u * NP + sel_par[k]];
    if (lstm) {
      c1cur[r * H + u] = c1n[u * NP + sel_par[k]];
      if (!tok_out) c0cur[r * H + u] = c0n[pr * H + u];
    }
  }
  DEC_STAMP(16);
}

// Teacher forcing (decode_seq, the training step): the same four-launch step as the beam search with beam = 1.  Before a step its
// inputs are assembled from the given token and the previous step's outputs (the encoder states / zero attention at step 0); the
// search's first step is the same assembly from bos (tgt == NULL: tok = col) and its clip's encoder states (source row r / beam).
//   x0[r] = [embed(tok), ctx_prev | 0, h0_prev], x1[r, 2H:3H] = h1_prev, and with c0_prev (LSTM, inference) c0cur / c1cur
__global__ void dec_prep_kernel(const float *__restrict__ emb, const int32_t *__restrict__ tgt, int ld, int col,
                                const float *__restrict__ ctx_prev, int ldc, const float *__restrict__ h0_prev, int ld0,
                                const float *__restrict__ h1_prev, int ld1, const float *__restrict__ c0_prev,
                                const float *__restrict__ c1_prev, float *__restrict__ x0, float *__restrict__ x1, int ldx1,
                                float *__restrict__ c0cur, float *__restrict__ c1cur, int beam, int H, int E) {
  const int r = blockIdx.x, K0 = E + 2 * H;
  const long rs = r / beam;
  const int tok = tgt ? tgt[(long)r * ld + col] : col;
  const float *e = emb + (long)(tok > 0 ? tok : 0) * E;
  for (int i = threadIdx.x; i < K0; i += blockDim.x)
    x0[(long)r * K0 + i] = i < E ? e[i] : i < E + H ? (ctx_prev ? ctx_prev[rs * ldc + i - E] : 0.f) : h0_prev[rs * ld0 + i - E - H];
  for (int u = threadIdx.x; u < H; u += blockDim.x) {
    x1[xidx(r, 2 * H + u, ldx1)] = h1_prev[rs * ld1 + u];
    if (c0_prev) { c0cur[(long)r * H + u] = c0_prev[rs * H + u]; c1cur[(long)r * H + u] = c1_prev[rs * H + u]; }
  }
}

// A decoder cell behind the attention (the last cell of teacher forcing, the cells between the first and the last one of
// num_layers > 2, gnmt.py:385-397; every such cell of the training step): gates on the stacked pre-activations g (R,4H) of
// x (R,3H) = [out of the layer below, attention, h_prev]; the new state goes to hn / cn.  Optional outputs, row stride ldo (the next
// layer's step input, or the rows the projection reads): out = the layer's output, dropout(h) (mask, training) + the layer's
// input with use_residual (gnmt.py:393-396); att_dst = the attention vector copied along.
__global__ void dec_cell_kernel(const float *__restrict__ g, const float *__restrict__ x, int lstm, const float *__restrict__ cprev,
                                float *__restrict__ hn, float *__restrict__ cn, const float *__restrict__ mask, int residual,
                                float *__restrict__ out, int ldo, float *__restrict__ att_dst, int R, int H) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)R * H) return;
  const long r = id / H;
  const int u = (int)(id - r * H);
  const float *gr = g + r * 4 * H;
  float h;
  if (lstm) {
    float c2;
    h = lstm_cell(gr[u], gr[H + u], gr[2 * H + u], gr[3 * H + u], cprev[id], c2);
    cn[id] = c2;
  } else {
    h = gru_cell(gr[u], gr[H + u], gr[2 * H + u], gr[3 * H + u], x[r * 3 * H + 2 * H + u]);
  }
  hn[id] = h;
  if (out) {
    const float hm = mask ? h * mask[id] : h;
    out[r * ldo + u] = residual ? hm + x[r * 3 * H + u] : hm;
  }
  if (att_dst) att_dst[r * ldo + u] = x[r * 3 * H + H + u];
}

// The recurrent state of such a layer for the next step: x[:, 2H:3H] = hn[row or its parent beam], ccur likewise (LSTM).
// parent == NULL (teacher forcing, or hn / cn = the encoder's states of the clip with `beam` rows per clip): by row / clip.
__global__ void dec_mid_state_kernel(const int32_t *__restrict__ parent, const float *__restrict__ hn,
                                     const float *__restrict__ cn, float *__restrict__ x, float *__restrict__ ccur,
                                     int from_clip, int beam, int R, int H) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)R * H) return;
  const long r = id / H;
  const int u = (int)(id - r * H);
  const long pr = from_clip ? r / beam : parent ? (r / beam) * beam + parent[r] : r;
  x[r * 3 * H + 2 * H + u] = hn[pr * H + u];
  if (cn) ccur[id] = cn[pr * H + u];
}

// y[i] = x[i] (* m[i]) (+ r[i]) over n elements (m / r optional; y may be x: a thread reads an element before it writes it)
__global__ void mul_add_kernel(const float *x, const float *__restrict__ m, const float *__restrict__ r, float *y, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = x[i];
  if (m) v *= m[i];
  if (r) v += r[i];
  y[i] = v;
}
// the same over (R, H) with row strides: out[r * ldo + u] = a[r * la + u] (* m[r * H + u]) (+ b[r * lb + u]); out may be a
__global__ void mul_add_rows_kernel(const float *a, int la, const float *__restrict__ m, const float *__restrict__ b, int lb, float *out,
                                    int ldo, int R, int H) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)R * H) return;
  const long r = id / H;
  const int u = (int)(id - r * H);
  float v = a[r * la + u];
  if (m) v *= m[id];
  if (b) v += b[r * lb + u];
  out[r * ldo + u] = v;
}

__global__ void beam_init_kernel(float *scores, int32_t *alive, int32_t *vlen, int32_t *tok, int32_t *samples, int L,
                                 int B, int beam, int bos) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= B * beam) return;
  scores[id] = (id % beam) == 0 ? 0.f : kNeg;
  alive[id] = 1;
  vlen[id] = 1;
  tok[id] = bos;
  samples[(long)id * L] = bos;
}

// The token prefixes of the final beams from the steps' (parent, word) back-pointers: sample[row][s] for s = steps .. 1 is the
// word chosen at step s by the row's ancestor of that step (-1 where a finished beam was carried over), sample[row][0] = bos -
// what copying the parent's prefix and appending the word at every step (BeamSearchSampler [EXT]) leaves behind.  One
// workgroup per clip; the clip's pointers pass through LDS in chunks of kSampChunk steps, newest first.
constexpr int kSampChunk = 256;
__global__ __launch_bounds__(256) void beam_samples_kernel(const int32_t *__restrict__ bp_par, const int32_t *__restrict__ bp_word,
                                                           int32_t *__restrict__ samples, int L, int steps, int R, int beam, int bos) {
  __shared__ int32_t par[kSampChunk * 16], word[kSampChunk * 16];
  const int b = blockIdx.x, t = threadIdx.x;
  int cur = t;
  int32_t *dst = samples + ((long)b * beam + (t < beam ? t : 0)) * L;
  for (int hi = steps; hi > 0; hi -= kSampChunk) {
    const int lo = hi > kSampChunk ? hi - kSampChunk : 0, n = hi - lo;
    __syncthreads();
    for (int i = t; i < n * beam; i += 256) {
      const int s = i / beam, k = i - s * beam;
      par[i] = bp_par[(long)(lo + s) * R + b * beam + k];
      word[i] = bp_word[(long)(lo + s) * R + b * beam + k];
    }
    __syncthreads();
    if (t < beam)
      for (int s = n - 1; s >= 0; --s) {
        dst[lo + s + 1] = word[s * beam + cur];
        cur = par[s * beam + cur];
      }
  }
  if (t < beam) dst[0] = bos;
}

__global__ void beam_finalize_kernel(const int32_t *alive, int32_t *vlen, int32_t *samples, int L, int last, int R,
                                     int eos) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= R) return;
  samples[(long)id * L + last] = alive[id] ? eos : -1;
  vlen[id] += alive[id] ? 1 : 0;
}

// ---- attention weights of the final hypotheses (tn_gnmt_beam_search_attention) ----
// While a search that asked for them runs, every step's dec_attention_kernel stores its R = B * beam rows into the step-major
// history hist (steps, R, T): 4 * max_length * max_batch * beam * max_src_len bytes at the handle's capacities (61.4 MB at
// config C5 with max_src_len 640), allocated by the first call that asks and never by a handle that does not.
// Afterwards the alignments are put together in two launches:
//   beam_att_rows_kernel   the walk of beam_samples_kernel again, keeping the ROW instead of the word: samples[b, k, i + 1]
//                          was emitted by step i in the row of the hypothesis' ancestor at that step, par[i][cur];
//                          rowtab (R, steps) holds that row, or -1 where no decoder step emitted the token (the -1 a
//                          finished beam carries)
//   beam_att_gather_kernel attention[b, k, i, :] = hist[i, rowtab[b * beam + k, i], :], exact zeros where the table says
//                          -1 and for i >= steps (behind the search's last step, which is also where the sampler appends
//                          <eos> to a beam still alive); one workgroup per (hypothesis, kAttGatherSteps steps), 16-byte
//                          accesses when T is a multiple of 4 and the output is 16-byte aligned.
__global__ __launch_bounds__(256) void beam_att_rows_kernel(const int32_t *__restrict__ bp_par, const int32_t *__restrict__ bp_word,
                                                            int32_t *__restrict__ rowtab, int steps, int R, int beam) {
  __shared__ int32_t par[kSampChunk * 16], word[kSampChunk * 16];
  const int b = blockIdx.x, t = threadIdx.x;
  int cur = t;
  int32_t *dst = rowtab + ((long)b * beam + (t < beam ? t : 0)) * steps;
  for (int hi = steps; hi > 0; hi -= kSampChunk) {
    const int lo = hi > kSampChunk ? hi - kSampChunk : 0, n = hi - lo;
    __syncthreads();
    for (int i = t; i < n * beam; i += 256) {
      const int s = i / beam, k = i - s * beam;
      par[i] = bp_par[(long)(lo + s) * R + b * beam + k];
      word[i] = bp_word[(long)(lo + s) * R + b * beam + k];
    }
    __syncthreads();
    if (t < beam)
      for (int s = n - 1; s >= 0; --s) {
        const int p = par[s * beam + cur];
        dst[lo + s] = word[s * beam + cur] >= 0 ? b * beam + p : -1;
        cur = p;
      }
  }
}

constexpr int kAttGatherSteps = 8;
template <bool VEC>
__global__ __launch_bounds__(256) void beam_att_gather_kernel(const float *__restrict__ hist, const int32_t *__restrict__ rowtab,
                                                              float *__restrict__ out, int steps, int R, int T, int LA) {
  const int hyp = blockIdx.x, i0 = blockIdx.y * kAttGatherSteps, i1 = min(LA, i0 + kAttGatherSteps), t = threadIdx.x;
  for (int i = i0; i < i1; ++i) {
    const int row = i < steps ? rowtab[(long)hyp * steps + i] : -1;
    float *d = out + ((long)hyp * LA + i) * T;
    const float *sp = row >= 0 ? hist + ((long)i * R + row) * T : nullptr;
    if (VEC) {
      for (int c = t; c < (T >> 2); c += 256)
        ((float4 *)d)[c] = sp ? ((const float4 *)sp)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int c = t; c < T; c += 256) d[c] = sp ? sp[c] : 0.f;
    }
  }
}

// MaskedSoftmaxCELoss [EXT gluonnlp]: per sample, mean over the L time steps of
// -log_softmax(logits[b,t])[label[b,t]] * (t < valid_len[b]).  One workgroup per sample.
__global__ __launch_bounds__(256) void masked_ce_kernel(const float *__restrict__ logits, const int32_t *__restrict__ labels,
                                                        int ldl, const int32_t *__restrict__ valid_len, float *__restrict__ loss,
                                                        int L, int V) {
  __shared__ float red[256];
  const int b = blockIdx.x, t = threadIdx.x;
  const int vl = valid_len[b];
  float total = 0.f;
  for (int s = 0; s < L && s < vl; ++s) {
    const float *z = logits + ((long)b * L + s) * V;
    float mx = -INFINITY;
    for (int v = t; v < V; v += 256) mx = fmaxf(mx, z[v]);
    red[t] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (t < o) red[t] = fmaxf(red[t], red[t + o]); __syncthreads(); }
    mx = red[0];
    __syncthreads();
    float sum = 0.f;
    for (int v = t; v < V; v += 256) sum += expf(z[v] - mx);
    red[t] = sum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (t < o) red[t] += red[t + o]; __syncthreads(); }
    if (t == 0) total += -(z[labels[(long)b * ldl + s]] - mx - logf(red[0]));
    __syncthreads();
  }
  if (t == 0) loss[b] = total / (float)L;
}

// ---- training step of the captioner (captioner_train.hip): the loss gradient and the backward kernels -----------------

// d loss / d logits for loss = sum over valid (b, t) of -log softmax(logits[b, t])[label] / (number of valid tokens);
// logits (B, L, V) as decode_seq lays them out, dlogits STEP-major (L, B, V) like every other per-step array here
__global__ __launch_bounds__(256) void trn_ce_bwd_kernel(const float *__restrict__ logits, const int32_t *__restrict__ labels,
                                                         int ldl, const int32_t *__restrict__ valid_len, int B, int L, int V,
                                                         float *__restrict__ dlogits, float *__restrict__ loss_rows) {
  __shared__ float red[256];
  const int i = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  int ntok = 0;
  for (int q = 0; q < B; ++q) ntok += min(max(valid_len[q], 0), L);
  const float *z = logits + ((long)b * L + i) * V;
  float *d = dlogits + ((long)i * B + b) * V;
  const bool valid = i < valid_len[b];
  float mx = -INFINITY;
  for (int v = t; v < V; v += 256) mx = fmaxf(mx, z[v]);
  red[t] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (t < o) red[t] = fmaxf(red[t], red[t + o]); __syncthreads(); }
  mx = red[0];
  __syncthreads();
  float sum = 0.f;
  for (int v = t; v < V; v += 256) sum += expf(z[v] - mx);
  red[t] = sum;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (t < o) red[t] += red[t + o]; __syncthreads(); }
  const float lse = mx + logf(red[0]);
  const int lab = labels[(long)b * ldl + i];
  const float sc = valid && ntok > 0 ? 1.0f / (float)ntok : 0.f;
  for (int v = t; v < V; v += 256) d[v] = (expf(z[v] - lse) - (v == lab ? 1.f : 0.f)) * sc;
  if (t == 0) loss_rows[(long)i * B + b] = valid ? (lse - z[lab]) * sc : 0.f;     // summed over (i, b) = the loss
}

// GRU cell backward on the stacked pre-activations g (R,4H) = [r, z, n_i2h, n_h2h]:
//   dh = sum of up to four addends (each (R,H) with its own row stride, null = absent)
//   dg (R,4H) = [d r, d z, d n, d n * r]   (the stacked weight matrix routes them to both branches)
//   dhz (R,H) = dh * z                     (the direct path to h_prev; the rest comes back through dg x W)
__global__ void trn_gru_bwd_kernel(const float *__restrict__ g, const float *__restrict__ hprev, int ldh,
                                   const float *a0, int l0, const float *a1, int l1, const float *a2, int l2,
                                   const float *a3, int l3, float *__restrict__ dg, float *dhz, int R, int H) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)R * H) return;
  const long r = id / H;
  const int u = (int)(id - r * H);
  const float *q = g + r * 4 * H;
  const float anh = q[3 * H + u];
  const GruGates a = gru_gates(q[u], q[H + u], q[2 * H + u], anh);
  const float rg = a.r, zg = a.z, ng = a.n;
  const float hp = hprev[r * ldh + u];
  float dh = 0.f;
  if (a0) dh += a0[r * l0 + u];
  if (a1) dh += a1[r * l1 + u];
  if (a2) dh += a2[r * l2 + u];
  if (a3) dh += a3[r * l3 + u];
  const float dn = dh * (1.f - zg) * (1.f - ng * ng);
  float *o = dg + r * 4 * H;
  o[u] = dn * anh * rg * (1.f - rg);
  o[H + u] = dh * (hp - ng) * zg * (1.f - zg);
  o[2 * H + u] = dn;
  o[3 * H + u] = dn * rg;
  dhz[id] = dh * zg;
}

// LSTM cell backward on the stacked pre-activations g (R,4H) = [i, f, g, o]: dc = dc_carry + dh o (1 - tanh^2 c);
// dg (R,4H); dcz = dc f (to c_prev); there is no direct path to h_prev (dhz = 0)
__global__ void trn_lstm_bwd_kernel(const float *__restrict__ g, const float *__restrict__ cprev, const float *__restrict__ cnew,
                                    const float *a0, int l0, const float *a1, int l1, const float *a2, int l2,
                                    const float *a3, int l3, const float *dcc, float *__restrict__ dg, float *dhz, float *dcz,
                                    int R, int H) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)R * H) return;
  const long r = id / H;
  const int u = (int)(id - r * H);
  const float *q = g + r * 4 * H;
  const LstmGates a = lstm_gates(q[u], q[H + u], q[2 * H + u], q[3 * H + u]);
  const float ig = a.i, fg = a.f, gg = a.g, og = a.o;
  const float tc = tanhf(cnew[id]);
  float dh = 0.f;
  if (a0) dh += a0[r * l0 + u];
  if (a1) dh += a1[r * l1 + u];
  if (a2) dh += a2[r * l2 + u];
  if (a3) dh += a3[r * l3 + u];
  const float dct = (dcc ? dcc[id] : 0.f) + dh * og * (1.f - tc * tc);
  float *o = dg + r * 4 * H;
  o[u] = dct * gg * ig * (1.f - ig);
  o[H + u] = dct * cprev[id] * fg * (1.f - fg);
  o[2 * H + u] = dct * ig * (1.f - gg * gg);
  o[3 * H + u] = dh * tc * og * (1.f - og);
  dhz[id] = 0.f;
  dcz[id] = dct * fg;
}

// Backward of one decoder step's attention (scaled Luong: ctx = sum_t w_t mem_t, w = softmax(s), s_t = q . kp_t, q = h0 / sqrt(H)) for
// one clip: dctx = up to two addends; dw_t = mem_t . dctx; ds = w (dw - w . dw); dq = sum_t ds_t kp_t -> dh0 = dq / sqrt(H).
// The step's share of d mem and d keyproj is NOT accumulated here (that was a read-modify-write of 2 T H floats per clip and
// step behind one workgroup, 123 us per step at config C5): the step only leaves ds (L,B,T) and dctx (L,B,H) behind, and
// trn_att_outer_kernel forms d mem = sum over steps of w (x) dctx and d keyproj = sum of ds (x) q once after the loop.
__global__ __launch_bounds__(kBeamThreads) void trn_att_bwd_kernel(const float *__restrict__ aw, const float *__restrict__ mem,
                                                                   const float *__restrict__ keyproj, const float *c0, int lc0, const float *c1, int lc1,
                                                                   const int32_t *__restrict__ valid_len, float *__restrict__ ds_out,
                                                                   float *__restrict__ dctx_out, float *__restrict__ dh0, int T, int H) {
  extern __shared__ float sm[];    // dctx[H] | ds[T] | part[16][H] | red[16]
  float *dctx = sm, *ds = dctx + H, *part = ds + T, *red = part + 16 * H;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int vl = min(max(valid_len[b], 0), T);
  const float inv = 1.0f / sqrtf((float)H);
  for (int u = t; u < H; u += kBeamThreads) {
    const float d = (c0 ? c0[(long)b * lc0 + u] : 0.f) + (c1 ? c1[(long)b * lc1 + u] : 0.f);
    dctx[u] = d;
    dctx_out[(long)b * H + u] = d;
  }
  __syncthreads();
  const float *w = aw + (long)b * T;
  const float *mv = mem + (long)b * T * H, *kp = keyproj + (long)b * T * H;
  // dw_t = mem_t . dctx: wave `wid` takes the steps wid, wid + 16, ...; a lane owns four units per 256 (16-byte loads along H),
  // eight steps in flight
  for (int s0 = wid; s0 < vl; s0 += 16 * 8) {
    float a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = 0.f;
    for (int u = 4 * lane; u < H; u += 256) {
      const float4 d = *(const float4 *)(dctx + u);
      float4 m[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int s = s0 + 16 * i;
        m[i] = s < vl ? *(const float4 *)(mv + (long)s * H + u) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) a[i] = fmaf(m[i].x, d.x, fmaf(m[i].y, d.y, fmaf(m[i].z, d.z, fmaf(m[i].w, d.w, a[i]))));
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float v = wave_sum(a[i]);
      if (lane == 0 && s0 + 16 * i < vl) ds[s0 + 16 * i] = v;
    }
  }
  __syncthreads();
  float pw = 0.f;
  for (int s = t; s < vl; s += kBeamThreads) pw += w[s] * ds[s];
  pw = wave_sum(pw);
  if (lane == 0) red[wid] = pw;
  __syncthreads();
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) dot += red[i];
  for (int s = t; s < T; s += kBeamThreads) {
    const float v = s < vl ? w[s] * (ds[s] - dot) : 0.f;
    ds_out[(long)b * T + s] = v;
    ds[s] = v;                  // each element is read (above) and written by the same thread
  }
  __syncthreads();
  // dq = sum_t ds_t kp_t: thread = (slice of the valid steps, four units), 16 partial sums per unit
  const int U4 = H >> 2, CG = step_groups(U4, 16), SG = kBeamThreads / CG;
  {
    const int sg = t / CG, sn = (vl + SG - 1) / SG, sa = sg * sn, sb = min(vl, sa + sn);
    for (int u4 = t % CG; u4 < U4; u4 += CG) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int s = sa; s < sb; s += 16) {
        float4 m[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) m[i] = s + i < sb ? *(const float4 *)(kp + (long)(s + i) * H + 4 * u4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float dv = s + i < sb ? ds[s + i] : 0.f;
          acc.x = fmaf(dv, m[i].x, acc.x); acc.y = fmaf(dv, m[i].y, acc.y); acc.z = fmaf(dv, m[i].z, acc.z); acc.w = fmaf(dv, m[i].w, acc.w);
        }
      }
      *(float4 *)(part + sg * H + 4 * u4) = acc;
    }
  }
  __syncthreads();
  for (int u = t; u < H; u += kBeamThreads) {
    float a = part[u];
    for (int g = 1; g < SG; ++g) a += part[g * H + u];
    dh0[(long)b * H + u] = a * inv;
  }
}

// d mem (B,T,H) = sum over the `steps` decoder steps of w_step (x) dctx_step, d keyproj = sum of ds_step (x) h0_step / sqrt(H):
// thread = (source step, four units), the steps' factors are (steps, B, T) / (steps, B, H) arrays (h0: pitch ldh per row).
__global__ __launch_bounds__(256) void trn_att_outer_kernel(const float *__restrict__ aw, const float *__restrict__ ds,
                                                            const float *__restrict__ dctx, const float *__restrict__ h0, int ldh,
                                                            float *__restrict__ dmem, float *__restrict__ dkp, int steps, int B, int T, int H) {
  const int b = blockIdx.y, u4 = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= T) return;
  const float inv = 1.0f / sqrtf((float)H);
  for (int u = 4 * u4; u < H; u += 256) {
    float4 am = make_float4(0.f, 0.f, 0.f, 0.f), ak = am;
    for (int l = 0; l < steps; ++l) {
      const long r = (long)l * B + b;
      const float w = aw[r * T + s], d = ds[r * T + s] * inv;
      const float4 c = *(const float4 *)(dctx + r * H + u), q = *(const float4 *)(h0 + r * ldh + u);
      am.x = fmaf(w, c.x, am.x); am.y = fmaf(w, c.y, am.y); am.z = fmaf(w, c.z, am.z); am.w = fmaf(w, c.w, am.w);
      ak.x = fmaf(d, q.x, ak.x); ak.y = fmaf(d, q.y, ak.y); ak.z = fmaf(d, q.z, ak.z); ak.w = fmaf(d, q.w, ak.w);
    }
    *(float4 *)(dmem + ((long)b * T + s) * H + u) = am;
    *(float4 *)(dkp + ((long)b * T + s) * H + u) = ak;
  }
}

// d embedding: rows of the step-major input gradients summed per token, in (step, row) order (deterministic)
__global__ void trn_emb_grad_kernel(const float *__restrict__ dx0, int K0, const int32_t *__restrict__ tgt, int ld, int B,
                                    int L, int E, int V, float *__restrict__ demb) {
  const int v = blockIdx.x;
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    float a = 0.f;
    for (int i = 0; i < L; ++i)
      for (int b = 0; b < B; ++b) {
        const int tok = tgt[(long)b * ld + i];
        if ((tok > 0 ? tok : 0) == v) a += dx0[((long)i * B + b) * K0 + e];
      }
    demb[(long)v * E + e] = a;
  }
}

// Gluon cell parameters <-> the stacked (4H, in+H) matrix of the step GEMM (GRU: rows r, z = [Wi | Wh], bias bi + bh;
// rows 2H..3H = [Wi_n | 0], bias bi_n; rows 3H..4H = [0 | Wh_n], bias bh_n)
// (LSTM: every row = [Wi | Wh], bias bi + bh)
__global__ void trn_stack_kernel(const float *__restrict__ wi, const float *__restrict__ wh, const float *__restrict__ bi,
                                 const float *__restrict__ bh, int in, int H, int lstm, float *__restrict__ wc,
                                 float *__restrict__ bc) {
  const int row = blockIdx.x, Kc = in + H;
  const int src_i = (lstm || row < 3 * H) ? row : -1, src_h = (lstm || row < 2 * H) ? row : row >= 3 * H ? row - H : -1;
  for (int k = threadIdx.x; k < Kc; k += blockDim.x)
    wc[(long)row * Kc + k] = k < in ? (src_i >= 0 ? wi[(long)src_i * in + k] : 0.f) : (src_h >= 0 ? wh[(long)src_h * H + k - in] : 0.f);
  if (threadIdx.x == 0) bc[row] = (src_i >= 0 ? bi[src_i] : 0.f) + (src_h >= 0 ? bh[src_h] : 0.f);
}
__global__ void trn_unstack_kernel(const float *__restrict__ dwc, const float *__restrict__ dbc, int in, int H, int lstm,
                                   float *__restrict__ dwi, float *__restrict__ dwh, float *__restrict__ dbi,
                                   float *__restrict__ dbh) {
  const int row = blockIdx.x, Kc = in + H;     // row of the Gluon (G*H, .) matrices
  const int ri = row, rh = (lstm || row < 2 * H) ? row : row + H;
  for (int k = threadIdx.x; k < Kc; k += blockDim.x) {
    if (k < in) dwi[(long)row * in + k] = dwc[(long)ri * Kc + k];
    else dwh[(long)row * H + k - in] = dwc[(long)rh * Kc + k];
  }
  if (threadIdx.x == 0) { dbi[row] = dbc[ri]; dbh[row] = dbc[rh]; }
}

// inverted dropout (gluon nn.Dropout in training mode): mask = keep ? 1/(1-p) : 0 from a counter-based hash (splitmix64),
// so a step's masks depend only on (seed, step counter, element index); y = x * mask
__global__ void trn_dropout_mask_kernel(float *__restrict__ mask, long n, float p, unsigned long long key) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long z = key + 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const float u = (float)(z >> 40) * (1.0f / 16777216.0f);      // uniform [0, 1)
  mask[i] = u < p ? 0.f : 1.0f / (1.0f - p);
}
__global__ void trn_dec_len_kernel(const int32_t *__restrict__ tgt_vl, int32_t *__restrict__ out, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) out[b] = tgt_vl[b] - 1;          // train_gnmt.py:331-332: the model and the loss see tgt_valid_length - 1
}

// a launch above 64 KiB of dynamic LDS needs the kernel's limit raised first (per device; the step kernels' limit is kStepLdsMax)
template <auto Kern>
int allow_lds(size_t bytes) {
  if (bytes > 64 * 1024)
    TN_SET_ATTR_ONCE_PER_DEVICE(TN_HIP_CHECK(hipFuncSetAttribute((const void *)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kStepLdsMax)));
  return TN_OK;
}
dim3 blocks256(long n) { return dim3((unsigned)((n + 255) / 256)); }
// the body of a plain launcher: one launch on `s` and its error
#define TN_LAUNCH(kern, grid, block, lds, ...)                     \
  do {                                                             \
    hipLaunchKernelGGL(kern, grid, block, lds, s, __VA_ARGS__);    \
    TN_HIP_CHECK(hipGetLastError());                               \
    return TN_OK;                                                  \
  } while (0)

}  // namespace

void pack_proj(const float *wp, const float *bp, int V, int H, std::vector<float> &wt, std::vector<float> &bpad) {
  const int vp = (V + 3) & ~3;
  wt.assign((size_t)H * vp, 0.f);
  for (int v = 0; v < V; ++v)
    for (int k = 0; k < H; ++k) wt[(size_t)k * vp + v] = wp[(size_t)v * H + k];
  bpad.assign(vp, 0.f);
  if (bp) memcpy(bpad.data(), bp, sizeof(float) * V);
}
std::vector<float> pack_wk4(const float *w, int N, int K) {
  std::vector<float> wk((size_t)K * N);
  for (int row = 0; row < N; ++row)
    for (int k = 0; k < K; ++k) wk[((size_t)(k >> 2) * N + row) * 4 + (k & 3)] = w[(size_t)row * K + k];
  return wk;
}

int launch_dec_attention(const DecAttentionArgs &a, hipStream_t s) {
  int split = att_split(a.T, a.H, kStepLdsMax);
  TN_REQUIRE(split > 0, "launch_dec_attention: 3 * max(hidden, source length) floats exceed the step kernel's 152 KiB of LDS");
  if (a.split_cap && a.split_cap < split) split = a.split_cap;
  const size_t lds = att_lds_bytes(a.T, a.H, split);
  TN_REQUIRE(lds <= kStepLdsMax, "launch_dec_attention: the capped split exceeds the step kernel's 152 KiB of LDS");
  TN_TRY(allow_lds<dec_attention_kernel>(lds));
  TN_LAUNCH(dec_attention_kernel, dim3(a.R), dim3(kBeamThreads), lds, a.g0, a.hprev, a.ldh, a.cprev, a.lstm ? 1 : 0, a.hn, a.cn, a.x1, a.ldx1,
            a.kpT, a.mem, a.valid_len, a.ctx, a.beam, 1, a.T, a.H, a.wsave, a.tok, a.par, a.ew, a.p0, split, a.wpitch);
}

int launch_dec_beam(const DecBeamArgs &a, hipStream_t s) {
  TN_REQUIRE(a.beam >= 1 && a.beam <= 16 && a.B >= 1, "launch_dec_beam: beam must be 1 to 16");
  const int H = a.H, R = a.B * a.beam, nbm = beam_nbm(a.beam);
  int split = beam_split(H, a.V, a.beam, kStepLdsMax);
  if (a.split_cap && a.split_cap < split) split = a.split_cap;
  const size_t lds = beam_lds_bytes(H, a.V, a.beam, split);
  TN_REQUIRE(lds <= kStepLdsMax, "launch_dec_beam: beam * (2*hidden + 2*vocab) floats exceed the step kernel's 152 KiB of LDS");
  LatGemmArgs gm{};
  int gemm_wgs = 0;
  if (a.p0) {
    gm = LatGemmArgs{a.x1, a.w1x, a.b1x, a.p0, a.K1, a.K1p, 4 * H, R, 4 * H, 2 * H};
    gemm_wgs = beam_gemm_wgs(R, H);
  }
  const size_t lds_launch = gemm_wgs && lds < kBeamTileLds ? kBeamTileLds : lds;      // the tiles' partial sums
#define TN_BEAM_LAUNCH(NBM)                                                                                                          \
  do {                                                                                                                               \
    TN_TRY(allow_lds<dec_beam_kernel<NBM>>(lds));                                                                                    \
    TN_LAUNCH(dec_beam_kernel<NBM>, dim3(a.B + gemm_wgs), dim3(kBeamThreads), lds_launch, a.g1, 4 * H, a.x1, a.K1, a.lstm ? 1 : 0,   \
              a.c1cur, a.wpT, a.bp, a.h0n, a.ctx, a.c0n, a.x0, a.c0cur, a.emb, H, a.E, a.V, a.beam, a.step, a.lp, a.prev_lp, a.eos,  \
              a.scores, a.alive, a.vlen, a.bp_par, a.bp_word, R, a.any_alive, a.hstate, a.parent_out, a.tok_out, a.B, gm, split);    \
  } while (0)
  if (nbm == 4) TN_BEAM_LAUNCH(4);
  else if (nbm == 5) TN_BEAM_LAUNCH(5);
  else if (nbm == 8) TN_BEAM_LAUNCH(8);
  else TN_BEAM_LAUNCH(16);
#undef TN_BEAM_LAUNCH
}

int launch_transpose_bth(const float *src, float *dst, int B, int T, int H, hipStream_t s) {
  TN_LAUNCH(transpose_bth_kernel, dim3((H + 31) / 32, (T + 31) / 32, B), dim3(256), 0, src, dst, T, H);
}
int launch_dec_prep(const float *emb, const int32_t *tgt, int ld, int col, const float *ctx_prev, int ldc, const float *h0_prev, int ld0,
                    const float *h1_prev, int ld1, const float *c0_prev, const float *c1_prev, float *x0, float *x1, int ldx1, float *c0cur,
                    float *c1cur, int beam, int R, int H, int E, hipStream_t s) {
  TN_LAUNCH(dec_prep_kernel, dim3(R), dim3(256), 0, emb, tgt, ld, col, ctx_prev, ldc, h0_prev, ld0, h1_prev, ld1, c0_prev, c1_prev, x0, x1, ldx1,
            c0cur, c1cur, beam, H, E);
}
int launch_dec_cell(const float *g, const float *x, bool lstm, const float *cprev, float *hn, float *cn, const float *mask, bool residual,
                    float *out, int ldo, float *att_dst, int R, int H, hipStream_t s) {
  TN_LAUNCH(dec_cell_kernel, blocks256((long)R * H), dim3(256), 0, g, x, lstm ? 1 : 0, cprev, hn, cn, mask, residual ? 1 : 0, out, ldo, att_dst, R, H);
}
int launch_dec_mid_state(const int32_t *parent, const float *hn, const float *cn, float *x, float *ccur, bool from_clip, int beam, int R, int H,
                         hipStream_t s) {
  TN_LAUNCH(dec_mid_state_kernel, blocks256((long)R * H), dim3(256), 0, parent, hn, cn, x, ccur, from_clip ? 1 : 0, beam, R, H);
}
int launch_mul_add(const float *x, const float *m, const float *r, float *y, long n, hipStream_t s) {
  TN_LAUNCH(mul_add_kernel, blocks256(n), dim3(256), 0, x, m, r, y, n);
}
int launch_mul_add_rows(const float *a, int la, const float *m, const float *b, int lb, float *out, int ldo, int R, int H, hipStream_t s) {
  TN_LAUNCH(mul_add_rows_kernel, blocks256((long)R * H), dim3(256), 0, a, la, m, b, lb, out, ldo, R, H);
}

int launch_beam_init(float *scores, int32_t *alive, int32_t *vlen, int32_t *tok, int32_t *samples, int L, int B, int beam, int bos, hipStream_t s) {
  TN_LAUNCH(beam_init_kernel, blocks256((long)B * beam), dim3(256), 0, scores, alive, vlen, tok, samples, L, B, beam, bos);
}
int launch_beam_samples(const int32_t *bp_par, const int32_t *bp_word, int32_t *samples, int L, int steps, int B, int beam, int bos, hipStream_t s) {
  TN_LAUNCH(beam_samples_kernel, dim3(B), dim3(256), 0, bp_par, bp_word, samples, L, steps, B * beam, beam, bos);
}
int launch_beam_finalize(const int32_t *alive, int32_t *vlen, int32_t *samples, int L, int last, int R, int eos, hipStream_t s) {
  TN_LAUNCH(beam_finalize_kernel, blocks256(R), dim3(256), 0, alive, vlen, samples, L, last, R, eos);
}
int launch_beam_attention(const int32_t *bp_par, const int32_t *bp_word, const float *hist, int32_t *rowtab, float *attention, int steps, int B,
                          int beam, int T, int LA, hipStream_t s) {
  const int R = B * beam;
  hipLaunchKernelGGL(beam_att_rows_kernel, dim3(B), dim3(256), 0, s, bp_par, bp_word, rowtab, steps, R, beam);
  const dim3 grid(R, (LA + kAttGatherSteps - 1) / kAttGatherSteps);
  if (T % 4 == 0 && ((uintptr_t)attention & 15) == 0)
    TN_LAUNCH(beam_att_gather_kernel<true>, grid, dim3(256), 0, hist, (const int32_t *)rowtab, attention, steps, R, T, LA);
  TN_LAUNCH(beam_att_gather_kernel<false>, grid, dim3(256), 0, hist, (const int32_t *)rowtab, attention, steps, R, T, LA);
}

int launch_masked_ce(const float *logits, const int32_t *labels, int ldl, const int32_t *valid_len, float *loss, int B, int L, int V, hipStream_t s) {
  TN_LAUNCH(masked_ce_kernel, dim3(B), dim3(256), 0, logits, labels, ldl, valid_len, loss, L, V);
}
int launch_trn_ce_bwd(const float *logits, const int32_t *labels, int ldl, const int32_t *valid_len, int B, int L, int V, float *dlogits,
                      float *loss_rows, hipStream_t s) {
  TN_LAUNCH(trn_ce_bwd_kernel, dim3(L, B), dim3(256), 0, logits, labels, ldl, valid_len, B, L, V, dlogits, loss_rows);
}
int launch_trn_gru_bwd(const float *g, const float *hprev, int ldh, const float *a0, int l0, const float *a1, int l1, const float *a2, int l2,
                       const float *a3, int l3, float *dg, float *dhz, int R, int H, hipStream_t s) {
  TN_LAUNCH(trn_gru_bwd_kernel, blocks256((long)R * H), dim3(256), 0, g, hprev, ldh, a0, l0, a1, l1, a2, l2, a3, l3, dg, dhz, R, H);
}
int launch_trn_lstm_bwd(const float *g, const float *cprev, const float *cnew, const float *a0, int l0, const float *a1, int l1, const float *a2,
                        int l2, const float *a3, int l3, const float *dcc, float *dg, float *dhz, float *dcz, int R, int H, hipStream_t s) {
  TN_LAUNCH(trn_lstm_bwd_kernel, blocks256((long)R * H), dim3(256), 0, g, cprev, cnew, a0, l0, a1, l1, a2, l2, a3, l3, dcc, dg, dhz, dcz, R, H);
}
int launch_trn_att_bwd(const float *aw, const float *mem, const float *keyproj, const float *c0, int lc0, const float *c1, int lc1,
                       const int32_t *valid_len, float *ds, float *dctx, float *dh0, int B, int T, int H, hipStream_t s) {
  const size_t lds = att_bwd_lds_bytes(T, H);
  TN_REQUIRE(lds <= kStepLdsMax, "launch_trn_att_bwd: 17 hidden + source length floats exceed the step kernel's 152 KiB of LDS");
  TN_TRY(allow_lds<trn_att_bwd_kernel>(lds));
  TN_LAUNCH(trn_att_bwd_kernel, dim3(B), dim3(kBeamThreads), lds, aw, mem, keyproj, c0, lc0, c1, lc1, valid_len, ds, dctx, dh0, T, H);
}
int launch_trn_att_outer(const float *aw, const float *ds, const float *dctx, const float *h0, int ldh, float *dmem, float *dkp, int steps, int B,
                         int T, int H, hipStream_t s) {
  TN_LAUNCH(trn_att_outer_kernel, dim3((T + 3) / 4, B), dim3(256), 0, aw, ds, dctx, h0, ldh, dmem, dkp, steps, B, T, H);
}
int launch_trn_emb_grad(const float *dx0, int K0, const int32_t *tgt, int ld, int B, int L, int E, int V, float *demb, hipStream_t s) {
  TN_LAUNCH(trn_emb_grad_kernel, dim3(V), dim3(64), 0, dx0, K0, tgt, ld, B, L, E, V, demb);
}
int launch_trn_stack(const float *wi, const float *wh, const float *bi, const float *bh, int in, int H, bool lstm, float *wc, float *bc, hipStream_t s) {
  TN_LAUNCH(trn_stack_kernel, dim3(4 * H), dim3(256), 0, wi, wh, bi, bh, in, H, lstm ? 1 : 0, wc, bc);
}
int launch_trn_unstack(const float *dwc, const float *dbc, int in, int H, bool lstm, float *dwi, float *dwh, float *dbi, float *dbh, hipStream_t s) {
  TN_LAUNCH(trn_unstack_kernel, dim3((lstm ? 4 : 3) * H), dim3(256), 0, dwc, dbc, in, H, lstm ? 1 : 0, dwi, dwh, dbi, dbh);
}
int launch_trn_dropout_mask(float *mask, long n, float p, unsigned long long key, hipStream_t s) {
  TN_LAUNCH(trn_dropout_mask_kernel, blocks256(n), dim3(256), 0, mask, n, p, key);
}
int launch_trn_dec_len(const int32_t *tgt_vl, int32_t *out, int B, hipStream_t s) {
  TN_LAUNCH(trn_dec_len_kernel, blocks256(B), dim3(256), 0, tgt_vl, out, B);
}
#ifdef TN_DEC_STAMPS
int read_dec_stamps(long long *out) {
  TN_HIP_CHECK(hipDeviceSynchronize());
  TN_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dec_stamps), sizeof(long long) * 24));
  return TN_OK;
}
#endif
