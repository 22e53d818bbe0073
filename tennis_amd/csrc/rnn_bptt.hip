// BPTT of the recurrent layer (rnn.hip's forward with its `save` output: GRU r | z | n | (W_hn h + b_hn), LSTM i | f | g | o | c_t per
// step).  Backward walks the steps in the reverse of each direction's own order inside one persistent workgroup per (direction, group
// of NB batch rows); the weight gradients are transposed GEMMs over all B*T rows afterwards (train.hip).  The kernels mirror the
// forward ones: the same routes (rnn.h), the same dot products (rnn_dot.h), one cell phase per cell type.
#include "common.h"
#include "train.h"
#include "rnn.h"
#include "rnn_dot.h"

namespace {

// The cell phase of BPTT step s for one (batch row bg, unit uu) of direction dir.  Reads the step's save record, h_prev from seq,
// dseq, and the gradient carried from the later step in *dh (LSTM: and *dc) - or dh_last (dc_last) at the row's last valid step.
// Writes the pre-activation gradients to dgi (GRU: and dgh, whose candidate block is d_n r), h_prev to hprev, the h2h gradients
// the dot product multiplies to the row's dgs [G*H] (LDS), and the carried gradient: GRU dh_t z into *dh (the W_hh^T term is
// added after the dot product), LSTM dc_t f into *dc.  A step at or past valid_len (or a row past B) leaves zeros and stores nothing.
template <int G>
__device__ __forceinline__ void rnn_bptt_cell(const float *__restrict__ seq, const float *__restrict__ save, const float *__restrict__ dseq,
                                              float *__restrict__ dgi, float *__restrict__ dgh, float *__restrict__ hprev, int B, int T,
                                              int H, int dirs, const int32_t *__restrict__ valid_len, const float *__restrict__ dh_last,
                                              const float *__restrict__ dc_last, int dir, int s, int bg, int uu, float *dh, float *dc,
                                              float *dgs) {
#pragma clang fp contract(off)   // the roundings below are the contract: a product is fused where fmaf says so and nowhere else
  const int GH = G * H;
  float d[G], carried = 0.f;
#pragma unroll
  for (int e = 0; e < G; ++e) d[e] = 0.f;
  const int vlen = bg < B ? (valid_len ? valid_len[bg] : T) : 0;
  if (s < vlen) {
    const int t = dir ? vlen - 1 - s : s;       // the reverse direction starts at the row's last valid step
    const int tp = dir ? t + 1 : t - 1;         // where h_prev of this step was emitted
    const long row = (long)bg * T + t;
    const float *sv = save + ((long)dir * B * T + row) * ((G + 1) * H);
    const bool lastp = s == vlen - 1;
    float *o1 = dgi + row * (dirs * GH) + dir * GH;
    if constexpr (G == 3) {
      const float r = sv[uu], z = sv[H + uu], n = sv[2 * H + uu], ghn = sv[3 * H + uu];
      const float hp = s > 0 ? seq[((long)bg * T + tp) * (dirs * H) + dir * H + uu] : 0.f;
      const float carry = (lastp && dh_last) ? dh_last[((long)dir * B + bg) * H + uu] : *dh;
      const float dht = carry + dseq[row * (dirs * H) + dir * H + uu];
      const float dn = dht * (1.f - z), dz = dht * (hp - n);
      carried = dht * z;
      const float d_n = dn * fmaf(-n, n, 1.f);
      d[1] = dz * z * (1.f - z);
      d[0] = d_n * ghn * r * (1.f - r);
      d[2] = d_n * r;
      float *o2 = dgh + row * (dirs * GH) + dir * GH;
      o1[uu] = d[0]; o1[H + uu] = d[1]; o1[2 * H + uu] = d_n;
      o2[uu] = d[0]; o2[H + uu] = d[1]; o2[2 * H + uu] = d[2];
      hprev[((long)dir * B * T + row) * H + uu] = hp;
    } else {
      const float ig = sv[uu], fg = sv[H + uu], gg = sv[2 * H + uu], og = sv[3 * H + uu], c2 = sv[4 * H + uu];
      float hp = 0.f, cp = 0.f;
      if (s > 0) {
        const long rp = (long)bg * T + tp;
        hp = seq[rp * (dirs * H) + dir * H + uu];
        cp = save[((long)dir * B * T + rp) * (5 * H) + 4 * H + uu];
      }
      const float tc = tanhf(c2);
      const float dht = ((lastp && dh_last) ? dh_last[((long)dir * B + bg) * H + uu] : *dh) + dseq[row * (dirs * H) + dir * H + uu];
      const float dct = fmaf(dht * og, fmaf(-tc, tc, 1.f), (lastp && dc_last) ? dc_last[((long)dir * B + bg) * H + uu] : *dc);
      d[3] = dht * tc * og * (1.f - og);
      d[0] = dct * gg * ig * (1.f - ig);
      d[1] = dct * cp * fg * (1.f - fg);
      d[2] = dct * ig * (1.f - gg * gg);
      carried = dct * fg;
      o1[uu] = d[0]; o1[H + uu] = d[1]; o1[2 * H + uu] = d[2]; o1[3 * H + uu] = d[3];
      hprev[((long)dir * B * T + row) * H + uu] = hp;
    }
  }
#pragma unroll
  for (int e = 0; e < G; ++e) dgs[e * H + uu] = d[e];
  *(G == 3 ? dh : dc) = carried;
}

// After the dot product: dh of (batch row, unit) from the G partial sums part[g][uu] of the row, g ascending.  GRU adds them to the
// dh_t z term the cell phase left; LSTM's dh is the sum alone.
template <int G>
__device__ __forceinline__ void rnn_bptt_gather(float *dh, const float *part, int H, int uu) {
  float sum = part[uu];
#pragma unroll
  for (int g = 1; g < G; ++g) sum += part[g * H + uu];
  *dh = G == 3 ? *dh + sum : sum;
}

// BPTT of one direction for NB batch rows: thread j = (gate block g, unit u).  As in rnn.hip's forward kernel the first KR values of
// the thread's W_hh column (loop-invariant over the steps) stay in registers, the rest is streamed 16 loads at a time, and small
// batches run one row per workgroup.  KL > 0 (NB = 1, H % 16 == 0): KL more weights in LDS, x through DPP (rnn_dot.h rnn_dot_big).
// LDS: dh [NB][H] | dc [NB][H] (LSTM) | dgs [NB][G*H] | part [NB][G][H] | wl [KL/4][G*H][4].
template <int G, int NB, int KR, int MAXT, int KL>
__global__ __launch_bounds__(MAXT) void rnn_bptt_kernel(
    const float *__restrict__ seq, const float *__restrict__ save, const float *__restrict__ dseq,
    const float *__restrict__ wh,                       // [dirs][G*H][H]
    float *__restrict__ dgi, float *__restrict__ dgh,   // [B*T][dirs*G*H]; dgh: GRU
    float *__restrict__ hprev,                          // [dirs][B*T][H]
    int B, int T, int H, int dirs,
    const int32_t *__restrict__ valid_len,              // [B] or null: steps >= valid_len never ran
    const float *__restrict__ dh_last, const float *__restrict__ dc_last) {   // [dirs][B][H] or null: d loss / d final h, c (LSTM)
  static_assert(KL == 0 || NB == 1, "the LDS share is built for one row per workgroup");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int GH = G * H;
  float *dh = lds;                                   // gradient flowing into h_t from the later step
  float *dc = dh + NB * H;                           // ... into c_t (LSTM)
  float *dgs = dh + (G == 4 ? 2 : 1) * NB * H;       // this step's h2h pre-activation gradients
  float *part = dgs + NB * GH;
  float *wl = part + NB * GH;
  const int j = threadIdx.x, dir = blockIdx.y, b0 = blockIdx.x * NB;
  const int g = j / H, u = j - g * H;
  const float *wrow = wh + (long)dir * GH * H + (long)g * H * H + u;   // W_hh[g*H + jj][u], jj = 0..H-1
  float wr[KR > 0 ? KR : 1];
#pragma unroll
  for (int k = 0; k < KR; ++k) wr[k] = wrow[(long)k * H];
  if constexpr (KL > 0) rnn_dot_fill_lds<KR, KL>(wl, GH, j, wrow, H);
  for (int i = j; i < NB * H; i += GH) {
    dh[i] = 0.f;
    if (G == 4) dc[i] = 0.f;
  }
  __syncthreads();
  for (int s = T - 1; s >= 0; --s) {          // reverse of the direction's own walking order
    for (int idx = j; idx < NB * H; idx += GH) {
      const int b = idx / H, uu = idx - b * H;
      rnn_bptt_cell<G>(seq, save, dseq, dgi, dgh, hprev, B, T, H, dirs, valid_len, dh_last, dc_last, dir, s, b0 + b, uu, dh + idx,
                       dc + idx, dgs + b * GH);
    }
    __syncthreads();
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.f;
    if constexpr (KL > 0) acc[0] = rnn_dot_big<KR, KL>(0.f, wr, wl, GH, j, wrow, H, dgs + g * H, H, (j & 3) * 4);
    else rnn_dot_stream<NB, KR>(acc, wr, wrow, H, dgs + g * H, GH, H);
#pragma unroll
    for (int b = 0; b < NB; ++b) part[(b * G + g) * H + u] = acc[b];
    __syncthreads();
    for (int idx = j; idx < NB * H; idx += GH) {
      const int b = idx / H, uu = idx - b * H;
      rnn_bptt_gather<G>(dh + idx, part + b * GH, H, uu);
    }
    __syncthreads();
  }
}

// The same for 1024 < G*H <= 2048: two gate rows per thread (rnn.h rnn_wide_route), as rnn.hip's wide forward kernel.  Thread j owns
// the rows j and j + blockDim.x of W_hh^T's product; a row past G*H works on the last row and stores nothing.  Both W_hh columns are
// streamed with 16 values in flight each.  Per row: one accumulator from 0, jj ascending - the sums of the kernel above, bit for bit.
// Its contract and LDS layout (no wl); the element-wise phases are its loops with the block size as stride.
template <int G, int NB>
__global__ __launch_bounds__(1024) void rnn_bptt_wide_kernel(
    const float *__restrict__ seq, const float *__restrict__ save, const float *__restrict__ dseq, const float *__restrict__ wh,
    float *__restrict__ dgi, float *__restrict__ dgh, float *__restrict__ hprev, int B, int T, int H, int dirs,
    const int32_t *__restrict__ valid_len, const float *__restrict__ dh_last, const float *__restrict__ dc_last) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int GH = G * H, nt = blockDim.x;
  float *dh = lds;
  float *dc = dh + NB * H;
  float *dgs = dh + (G == 4 ? 2 : 1) * NB * H;
  float *part = dgs + NB * GH;
  const int j = threadIdx.x, dir = blockIdx.y, b0 = blockIdx.x * NB;
  const bool own[2] = {j < GH, j + nt < GH};
  int gofs[2], pofs[2];             // where the row's gate block starts in dgs; where its sum goes in a batch row's part
  const float *wrow[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int rr = min(j + r * nt, GH - 1), g = rr / H, u = rr - g * H;
    gofs[r] = g * H;
    pofs[r] = rr;                   // (b * G + g) * H + u = b * GH + rr
    wrow[r] = wh + (long)dir * GH * H + (long)g * H * H + u;   // W_hh[g*H + jj][u], jj = 0..H-1
  }
  for (int i = j; i < NB * H; i += nt) {
    dh[i] = 0.f;
    if (G == 4) dc[i] = 0.f;
  }
  __syncthreads();
  for (int s = T - 1; s >= 0; --s) {
    for (int idx = j; idx < NB * H; idx += nt) {
      const int b = idx / H, uu = idx - b * H;
      rnn_bptt_cell<G>(seq, save, dseq, dgi, dgh, hprev, B, T, H, dirs, valid_len, dh_last, dc_last, dir, s, b0 + b, uu, dh + idx,
                       dc + idx, dgs + b * GH);
    }
    __syncthreads();
    float acc[2][NB];
    rnn_dot_stream2<NB>(acc, wrow, dgs, gofs, GH, H);
#pragma unroll
    for (int r = 0; r < 2; ++r)
      if (own[r]) {
#pragma unroll
        for (int b = 0; b < NB; ++b) part[b * GH + pofs[r]] = acc[r][b];
      }
    __syncthreads();
    for (int idx = j; idx < NB * H; idx += nt) {
      const int b = idx / H, uu = idx - b * H;
      rnn_bptt_gather<G>(dh + idx, part + b * GH, H, uu);
    }
    __syncthreads();
  }
}

// rows per workgroup / register-resident prefix / big split / LDS: rnn_route and rnn_wide_route (rnn.h), the policy of
// launch_rnn_recurrent, whose `save` these kernels read
template <int G>
int rnn_bptt_launch(const float *seq, const float *save, const float *dseq, const float *wh, float *dgi, float *dgh, float *hprev, int B,
                    int T, int H, hipStream_t s, int dirs, const int32_t *valid_len, const float *dh_last, const float *dc_last) {
#define TN_BPTT_LAUNCH(KERNEL, GRID, BLOCK, LDS) \
  hipLaunchKernelGGL((KERNEL), GRID, BLOCK, LDS, s, seq, save, dseq, wh, dgi, dgh, hprev, B, T, H, dirs, valid_len, dh_last, dc_last)
#define TN_BPTT_RAISE_LDS(KERNEL) \
  TN_SET_ATTR_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024))
  if (rnn_takes_wide(G, H)) {   // past gates*hidden = 1024 (or under tn_dbg_rnn_force_wide): two gate rows per thread
    const tn_rnn_wide_route wr = rnn_wide_route(G, B, H, dirs);
    const dim3 wgrid((B + wr.nb - 1) / wr.nb, dirs), wblock(wr.threads);
    if (wr.nb == 4) {           // 80 KiB at LSTM H = 512: above what a launch may ask for unraised
      TN_BPTT_RAISE_LDS((rnn_bptt_wide_kernel<G, 4>));
      TN_BPTT_LAUNCH((rnn_bptt_wide_kernel<G, 4>), wgrid, wblock, wr.lds_bwd);
    } else {
      TN_BPTT_LAUNCH((rnn_bptt_wide_kernel<G, 1>), wgrid, wblock, wr.lds_bwd);
    }
    rnn_count_wide_launch();
    TN_HIP_CHECK(hipGetLastError());
    return TN_OK;
  }
  const tn_rnn_route route = rnn_route(G, B, H, dirs);
  const dim3 grid((B + route.nb - 1) / route.nb, dirs), block(G * H);
  if (route.big) {              // the column does not fit the registers: registers + LDS + stream (rnn_dot.h)
    constexpr tn_rnn_big_split sp = rnn_big_split(G);
    TN_BPTT_RAISE_LDS((rnn_bptt_kernel<G, 1, sp.kr, sp.threads, sp.kl>));
    TN_BPTT_LAUNCH((rnn_bptt_kernel<G, 1, sp.kr, sp.threads, sp.kl>), grid, block, route.lds_bwd);
  }
  else if (route.nb == 4) TN_BPTT_LAUNCH((rnn_bptt_kernel<G, 4, 0, 1024, 0>), grid, block, route.lds_bwd);
  else if (route.kr == 128) TN_BPTT_LAUNCH((rnn_bptt_kernel<G, 1, 128, 512, 0>), grid, block, route.lds_bwd);
  else if (route.kr == 96) TN_BPTT_LAUNCH((rnn_bptt_kernel<G, 1, 96, 768, 0>), grid, block, route.lds_bwd);
  else if (route.kr == 64) TN_BPTT_LAUNCH((rnn_bptt_kernel<G, 1, 64, 1024, 0>), grid, block, route.lds_bwd);
  else TN_BPTT_LAUNCH((rnn_bptt_kernel<G, 1, 0, 1024, 0>), grid, block, route.lds_bwd);
#undef TN_BPTT_RAISE_LDS
#undef TN_BPTT_LAUNCH
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

}  // namespace

int launch_rnn_bptt(int gates, const float *seq, const float *save, const float *dseq, const float *wh, float *dgi, float *dgh,
                    float *hprev, int B, int T, int H, hipStream_t s, int dirs, const int32_t *valid_len, const float *dh_last,
                    const float *dc_last) {
  TN_REQUIRE(gates == 3 || gates == 4, "train: gates must be 3 or 4");
  TN_REQUIRE(H > 0 && gates * H <= 2048 && H % 4 == 0, "train: gates*hidden must be <= 2048 and hidden % 4 == 0");
  return gates == 3 ? rnn_bptt_launch<3>(seq, save, dseq, wh, dgi, dgh, hprev, B, T, H, s, dirs, valid_len, dh_last, dc_last)
                    : rnn_bptt_launch<4>(seq, save, dseq, wh, dgi, dgh, hprev, B, T, H, s, dirs, valid_len, dh_last, dc_last);
}
