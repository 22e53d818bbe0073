// Events from per-frame logits (tn_event_decoder_*, include/tennis_hip.h; docs/kernels.md "Event decoding").
//   p[m]        = softmax(logits[clamp(rows[m], 0, N-1)])          max subtracted, expf, sum in ascending c, one division per value
//   score[m, c] = (sum_{j = lo..hi} p[j, c]) / (hi - lo + 1)       j ascending; lo = max(m - h, first position of m's video),
//                                                                  hi = min(m + h, last position of m's video), h = (width - 1) / 2
//   label[m]    = first arg-max of score[m],  conf[m] = score[m, label[m]]
//   an event    = a maximal stretch of positions of one video with one label: first, last, cls, peak = max conf, score = mean conf
// Four plain launches on one stream; no workgroup waits on another, no float atomics, and no value depends on the grid:
//   1 event_score_kernel    one workgroup per tile of kEventTile positions: gathers the tile's rows plus h + 1 positions in front and h
//                           behind into LDS, softmax once per staged row, every position sums its window from LDS; writes label, conf,
//                           the run-start flags and the tile's flag count.  The position in front of the tile is decoded once more here,
//                           so that the flag of the tile's first position reads no other workgroup's output.
//   2 event_scan_kernel     ONE workgroup: exclusive scan of the tile counts in pieces of kEventScanBlock, writes the event count K
//   3 event_scatter_kernel  one workgroup per tile: ev_first[offset of the tile + rank in the tile] = position of a set flag
//   4 event_reduce_kernel   one wave per event (grid-stride over K, which only the device knows): lane l takes the positions
//                           first + l, first + l + 64, ... in ascending order, then a six-level xor tree (32, 16, ..., 1) as
//                           class_maps_kernel's; score = sum / length.  The order depends on the event's own positions only.
//
// With a switch cost (tn_event_decoder_run_switch; docs/kernels.md "Event decoding with a switch cost") label comes from the path that
// maximises sum_m e[m, label[m]] - cost * (changes of label inside a video), e[m, c] = q[c] - max_c q[c]:
//   forward   v_0 = e_0;  stay_t[c] = (v_{t-1}[c] >= -cost);  u_t[c] = e_t[c] + max(v_{t-1}[c], -cost);  v_t = u_t - max_c u_t;
//             a_t = first arg-max of v_t          (fp32, positions in order: the sequential order is the definition)
//   back      label[T-1] = a_{T-1};  label[t-1] = stay_t[label[t]] ? label[t] : a_{t-1}
//   conf[m]   = softmax(q)[label[m]], computed as event_score_kernel computes p
// With a transition matrix (tn_event_decoder_run_transitions; docs/kernels.md "Event decoding with a transition matrix") the path
// maximises sum_m e[m, label[m]] + sum_{m not a video's first} T[label[m-1], label[m]], T (C, C) with entries <= 0 or -inf and a
// finite diagonal:
//   forward   v_0 = e_0;  w_t[c] = max_p (v_{t-1}[p] + T[p, c]);  b_t[c] = c if v_{t-1}[c] + T[c, c] attains w_t[c], else the smallest
//             p that does;  u_t[c] = e_t[c] + w_t[c];  v_t = u_t - max_c u_t;  a_t = first arg-max of v_t
//   back      label[T-1] = a_{T-1};  label[t-1] = b_t[label[t]]
// Either path is nine plain launches (and the copy of the matrix): the video bounds are the set flags of `start`, found with the
// scan and scatter above (find_videos); then
//   viterbi_forward_kernel<ONE_ROW, TRANS>  one workgroup per video (grid-stride over the videos, whose number only the device knows).
//                             Wave 0 walks the chain, lane c holding v[c]; the maximum is a DPP all-reduce, the arg-max one ballot.
//                             Waves 1..3 gather the next tile of kViterbiTile rows and store e into the other half of the LDS.
//                             TRANS selects the step and what a position leaves behind: the stay mask, one ballot, kept in a register;
//                             or b_t, with the column T[:, c] in registers, v[p] a scalar from readlane and the C candidates of a
//                             step independent - a tile's back-pointers go through LDS and leave as whole rows of a fixed pitch.
//   viterbi_backtrack_kernel  one wave per video, tiles back to front: lane j holds stay_{t+1} and a_t of its position, the tile in
//                             front is in flight while the wave walks this one with scalar selects
//   viterbi_trans_backtrack_kernel  the same walk over b_t: the rows of the tile in front are in flight while the wave walks this
//                             one, one dependent LDS byte read per position
//   event_flag_kernel<true>   one thread per position: conf, the run-start flags and the tile counts - what event_score_kernel
//                             leaves behind, so that scan, scatter and reduce run unchanged (emit_events)
// With posteriors (tn_event_decoder_run_posteriors; docs/kernels.md "Event scores from posteriors") label is the path under the
// matrix as above and conf[m] = gamma_m[label[m]], gamma_t[c] = P(label_t = c | every position of the video) under the same HMM, from
// the forward-backward recurrences in the log domain, LSE(x) = mx + ln sum_i exp(x_i - mx) in ascending i:
//   forward   a_0 = e_0;  a_t[c] = e_t[c] + LSE_p(ah_{t-1}[p] + T[p, c]);  ah_t = a_t - max_c a_t
//   backward  b_{L-1} = 0;  b_t[p] = LSE_c(T[p, c] + (e_{t+1}[c] + bh_{t+1}[c]));  bh_t = b_t - max_p b_t
//   gamma_t   = softmax_c(ah_t + bh_t)
// Two more launches between the backtrack and the flags:
//   hmm_chain_kernel<ONE_ROW>  one workgroup per chain, two chains per video (even workgroups walk forward, odd ones backward, so
//                             that both directions of a video run at once); wave 0 walks, waves 1..3 stage e as for the Viterbi
//                             kernel, backward in descending tiles.  Every position leaves ah_t or bh_t as a row of the workspace.
//   hmm_posterior_kernel<ONE_ROW>  one thread per position: gamma, and conf = gamma[label].  event_flag_kernel<true> runs in front
//                             of it unchanged (its conf is overwritten), scan, scatter and reduce behind it.
#include "common.h"

#include <cmath>

namespace {

constexpr int kEventTile = 128;          // positions per workgroup of the score and scatter kernels
constexpr int kEventScanBlock = 1024;    // tile counts the scan workgroup takes per step (any number of tiles: it loops)
constexpr int kEventMaxHalf = 31;        // width <= 63
constexpr int kEventThreads = 256;

__host__ __device__ constexpr int event_ldp(int C) { return C | 1; }      // odd row stride: lanes reading one column of consecutive rows hit distinct banks

// dynamic LDS: p[S][ldp] fp32 | row[S] int32 | begins[S] int32 | lab[kEventTile + 1] int32 | wcnt[4] int32,  S = kEventTile + 2 h + 1
__host__ __device__ constexpr size_t event_lds_bytes(int C, int h) {
  return ((size_t)(kEventTile + 2 * h + 1) * (event_ldp(C) + 2) + kEventTile + 1 + 4) * 4;
}
static_assert(event_lds_bytes(64, kEventMaxHalf) <= 64 * 1024, "the score kernel stays inside the default LDS limit");

template <bool VEC4>
__global__ __launch_bounds__(kEventThreads) void event_score_kernel(const float *__restrict__ logits, int N, int C, const int32_t *__restrict__ rows,
                                                                    const int32_t *__restrict__ start, int M, int h, int32_t *__restrict__ label,
                                                                    float *__restrict__ conf, uint8_t *__restrict__ flags,
                                                                    int32_t *__restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) float event_lds[];
  const int S = kEventTile + 2 * h + 1, ldp = event_ldp(C);
  float *p = event_lds;
  int *srow = (int *)(p + (size_t)S * ldp);
  int *sbeg = srow + S;
  int *slab = sbeg + S;
  int *wcnt = slab + kEventTile + 1;
  const int tid = threadIdx.x;
  const int t0 = blockIdx.x * kEventTile;
  const int m0 = t0 - h - 1;                       // the position staged row 0 stands for
  // staged row s = position m0 + s: its logit row (-1: no such position) and whether a video begins there.  A position past the end
  // counts as a beginning, so that no window runs over it; position 0 always is one.
  for (int s = tid; s < S; s += kEventThreads) {
    const int m = m0 + s;
    int r = -1, b = 1;
    if (m >= 0 && m < M) {
      r = min(max(rows[m], 0), N - 1);
      b = (m == 0 || start[m] != 0) ? 1 : 0;
    }
    srow[s] = r;
    sbeg[s] = b;
  }
  __syncthreads();
  // the logits of the staged rows, consecutive lanes on consecutive addresses of a row
  if constexpr (VEC4) {
    const int c4 = C >> 2;
    for (int i = tid; i < S * c4; i += kEventThreads) {
      const int s = i / c4, k = i - s * c4, r = srow[s];
      if (r >= 0) {
        const float4 v = ((const float4 *)(logits + (size_t)r * C))[k];
        float *d = p + (size_t)s * ldp + 4 * k;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      }
    }
  } else {
    for (int i = tid; i < S * C; i += kEventThreads) {
      const int s = i / C, c = i - s * C, r = srow[s];
      if (r >= 0) p[(size_t)s * ldp + c] = logits[(size_t)r * C + c];
    }
  }
  __syncthreads();
  // softmax, once per staged row
  for (int s = tid; s < S; s += kEventThreads) {
    if (srow[s] < 0) continue;
    float *q = p + (size_t)s * ldp;
    float mx = q[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, q[c]);
    float sum = 0.f;
    for (int c = 0; c < C; ++c) {
      const float e = expf(q[c] - mx);
      q[c] = e;
      sum += e;
    }
    for (int c = 0; c < C; ++c) q[c] = q[c] / sum;
  }
  __syncthreads();
  // thread i decodes position t0 - 1 + i: i = 0 is the position in front of the tile (its label only)
  const int m = t0 - 1 + tid;
  const bool live = tid <= kEventTile && m >= 0 && m < M;
  int best = 0;
  float bestv = 0.f;
  if (live) {
    const int sc = tid + h;                        // the staged row of position m
    int lo = sc, hi = sc;
    for (int k = 0; k < h && !sbeg[lo]; ++k) --lo;
    for (int k = 0; k < h && !sbeg[hi + 1]; ++k) ++hi;
    const int n = hi - lo + 1;
    const float fn = (float)n;
    for (int c = 0; c < C; ++c) {
      float acc = p[(size_t)lo * ldp + c];
      for (int j = lo + 1; j <= hi; ++j) acc += p[(size_t)j * ldp + c];
      const float v = n > 1 ? acc / fn : acc;
      if (c == 0 || v > bestv) {
        bestv = v;
        best = c;
      }
    }
    slab[tid] = best;
  }
  __syncthreads();
  int f = 0;
  if (live && tid >= 1) {
    f = (sbeg[tid + h] || slab[tid - 1] != best) ? 1 : 0;       // (sbeg of position 0 is set: slab[0] is never read unwritten)
    label[m] = best;
    conf[m] = bestv;
    flags[m] = (uint8_t)f;
  }
  const int nw = __popcll(__ballot(f));
  if ((tid & 63) == 0) wcnt[tid >> 6] = nw;
  __syncthreads();
  if (tid == 0) counts[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// exclusive scan of counts[0, nb) -> offsets, the total -> *count; one workgroup, pieces of kEventScanBlock
__global__ __launch_bounds__(kEventScanBlock) void event_scan_kernel(const int32_t *__restrict__ counts, int nb, int32_t *__restrict__ offsets,
                                                                     int32_t *__restrict__ count) {
  __shared__ int wsum[kEventScanBlock / 64];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += kEventScanBlock) {
    const int i = base + tid;
    const int v = i < nb ? counts[i] : 0;
    int x = v;                                     // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int before = carry_s;
    for (int k = 0; k < w; ++k) before += wsum[k];
    if (i < nb) offsets[i] = before + x - v;
    __syncthreads();
    if (tid == kEventScanBlock - 1) carry_s = before + x;
    __syncthreads();
  }
  if (tid == 0) *count = carry_s;
}

__global__ __launch_bounds__(kEventTile) void event_scatter_kernel(const uint8_t *__restrict__ flags, int M, const int32_t *__restrict__ offsets,
                                                                   int32_t *__restrict__ ev_first) {
  __shared__ int wcnt[kEventTile / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int m = blockIdx.x * kEventTile + tid;
  const int f = m < M ? flags[m] : 0;
  const unsigned long long mask = __ballot(f);
  if (lane == 0) wcnt[w] = __popcll(mask);
  __syncthreads();
  if (f) {
    int rank = __popcll(mask & ((1ull << lane) - 1ull));
    for (int k = 0; k < w; ++k) rank += wcnt[k];
    ev_first[offsets[blockIdx.x] + rank] = m;
  }
}

__global__ __launch_bounds__(256) void event_reduce_kernel(const int32_t *__restrict__ label, const float *__restrict__ conf, int M,
                                                           const int32_t *__restrict__ count, const int32_t *__restrict__ ev_first,
                                                           int32_t *__restrict__ ev_last, int32_t *__restrict__ ev_cls,
                                                           float *__restrict__ ev_score, float *__restrict__ ev_peak) {
  const int lane = threadIdx.x & 63;
  const int K = *count;
  const int waves = gridDim.x * 4;
  for (int e = blockIdx.x * 4 + (threadIdx.x >> 6); e < K; e += waves) {      // (whole waves; the kernel has no barrier)
    const int first = ev_first[e];
    const int last = (e + 1 < K ? ev_first[e + 1] : M) - 1;
    float sum = 0.f, peak = 0.f;                   // (a conf is a mean of probabilities: > 0)
#pragma unroll 4
    for (int j = first + lane; j <= last; j += 64) {
      const float v = conf[j];
      sum += v;
      peak = fmaxf(peak, v);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      sum += __shfl_xor(sum, d, 64);
      peak = fmaxf(peak, __shfl_xor(peak, d, 64));
    }
    if (lane == 0) {
      ev_last[e] = last;
      ev_cls[e] = label[first];
      ev_score[e] = sum / (float)(last - first + 1);
      ev_peak[e] = peak;
    }
  }
}

// ---- the two path decoders ----

constexpr int kViterbiTile = 64;         // positions of a video per step of the forward and backtrack kernels
constexpr int kViterbiThreads = 256;     // forward: wave 0 walks, the other waves stage
constexpr int kViterbiStageWaves = kViterbiThreads / 64 - 1;
constexpr int kViterbiRowsPerWave = (kViterbiTile + kViterbiStageWaves - 1) / kViterbiStageWaves;
constexpr int kViterbiChunk = 8;         // positions the walking wave reads ahead of the chain
constexpr int kViterbiMaxGrid = 1024;    // workgroups of the two chain kernels (any number of videos: they loop)
constexpr int kEventMaxClasses = 64;     // one lane per class

// static LDS of the forward kernel: two tiles of e, rows kEventMaxClasses wide whatever C is (the lanes past C hold -inf)
__host__ __device__ constexpr size_t viterbi_lds_bytes() { return (size_t)2 * kViterbiTile * kEventMaxClasses * 4; }
static_assert(viterbi_lds_bytes() <= 64 * 1024, "the forward kernel stays inside the default LDS limit");
static_assert(kViterbiTile == 64, "a tile's stay masks and arg-maxima are kept one position per lane");
static_assert(kViterbiTile % kViterbiChunk == 0, "whole chunks");

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}

__device__ __forceinline__ float lane_f32(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }

// The maximum over the wave, the same in every lane; call it with all 64 lanes active.  A maximum is exact, so its order is free.
// ONE_ROW: only lanes 0..15 can hold it (C <= 16, the others hold -inf).
template <bool ONE_ROW>
__device__ __forceinline__ float wave_max(float x) {
  x = fmaxf(x, dpp_f32<0xB1>(x));        // quad_perm [1, 0, 3, 2]
  x = fmaxf(x, dpp_f32<0x4E>(x));        // quad_perm [2, 3, 0, 1]
  x = fmaxf(x, dpp_f32<0x141>(x));       // row_half_mirror
  x = fmaxf(x, dpp_f32<0x140>(x));       // row_mirror: every lane holds the maximum of its row of 16
  if constexpr (ONE_ROW) return lane_f32(x, 0);
  return fmaxf(fmaxf(lane_f32(x, 0), lane_f32(x, 16)), fmaxf(lane_f32(x, 32), lane_f32(x, 48)));
}

// e of the positions t0 + s, s < kViterbiTile, that lie before ve -> buf[s][lane]; wave w (1..3) takes s = w - 1, w + 2, ...  All its
// loads are issued before the first maximum, so that a tile costs two global round trips, not two per row.
// The same for values that are all <= 0 (-inf and either zero included), as every u of the recurrence is: e <= 0 and max(v, -cost) <= 0.
// Such floats are ordered against their bit patterns taken as unsigned integers, so their maximum is the unsigned minimum of the
// patterns - one v_min_u32 with the DPP operand folded in where fmaxf costs a move and two v_max_f32 (hipcc canonicalises both
// operands), and scalar minima for the four rows.  +0 and -0 both stand for zero; which of them comes back changes no sum and no
// comparison below.
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned x) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true);
}

__device__ __forceinline__ unsigned lane_u32(unsigned x, int l) { return (unsigned)__builtin_amdgcn_readlane((int)x, l); }

__device__ __forceinline__ float max_nonpos(float a, float b) { return __uint_as_float(min(__float_as_uint(a), __float_as_uint(b))); }

template <bool ONE_ROW>
__device__ __forceinline__ float wave_max_nonpos(float v) {
  unsigned x = __float_as_uint(v);
  x = min(x, dpp_u32<0xB1>(x));
  x = min(x, dpp_u32<0x4E>(x));
  x = min(x, dpp_u32<0x141>(x));
  x = min(x, dpp_u32<0x140>(x));
  if constexpr (ONE_ROW) return __uint_as_float(lane_u32(x, 0));
  return __uint_as_float(min(min(lane_u32(x, 0), lane_u32(x, 16)), min(lane_u32(x, 32), lane_u32(x, 48))));
}

template <bool ONE_ROW>
__device__ __forceinline__ void viterbi_stage(float (*buf)[kEventMaxClasses], int t0, int ve, const float *__restrict__ logits, int N, int C,
                                              const int32_t *__restrict__ rows, int wave, int lane) {
  // no load sits under a branch: a position past the video reads the video's last one, a lane past C reads class C - 1
  const int row = min(max(rows[min(t0 + lane, ve - 1)], 0), N - 1);          // lane l: the logit row of position t0 + l
  const int s0 = __builtin_amdgcn_readfirstlane(wave) - 1, col = min(lane, C - 1);
  float q[kViterbiRowsPerWave];
#pragma unroll
  for (int i = 0; i < kViterbiRowsPerWave; ++i) {
    const int r = __builtin_amdgcn_readlane(row, min(s0 + i * kViterbiStageWaves, kViterbiTile - 1));
    q[i] = logits[(size_t)r * C + col];
  }
#pragma unroll
  for (int i = 0; i < kViterbiRowsPerWave; ++i) {
    const int s = s0 + i * kViterbiStageWaves;
    if (s < kViterbiTile && t0 + s < ve) {                                    // (wave-uniform)
      const float x = lane < C ? q[i] : -INFINITY;
      buf[s][lane] = x - wave_max<ONE_ROW>(x);
    }
  }
}

// bytes of a position's row of back-pointers: one row of lanes up to 16 classes, one lane per class above
template <bool ONE_ROW>
__host__ __device__ constexpr int trans_pitch() { return ONE_ROW ? 16 : kEventMaxClasses; }

struct video_span {
  int vb, ve, ntiles;      // positions [vb, ve) in tiles of kViterbiTile, counted from vb
};

__device__ __forceinline__ video_span video_of(const int32_t *__restrict__ vid_first, int V, int vid, int M) {
  const int vb = vid_first[vid], ve = vid + 1 < V ? vid_first[vid + 1] : M;
  return {vb, ve, (ve - vb + kViterbiTile - 1) / kViterbiTile};
}

// TRANS = false, the switch cost: a position leaves its stay mask (one ballot, kept in a register) in `stay`.
// TRANS = true, the matrix: on the chain lane c holds v[c], the column T[:, c] (tc, -inf past C: such a predecessor is never chosen)
// and T[c, c].  A step forms the candidates v[p] + T[p, c] in ascending p from v[p] as a scalar and keeps the first maximum (strict
// comparison), then lets staying win a tie; a position leaves its row of b_t in `back`, through sb.  A NaN compares false
// everywhere, so every stored index is in [0, C) whatever the floats are.
// Every u is <= 0 or -inf on either path (e <= 0, max(v, -cost) <= 0, T <= 0), so the wave maximum is wave_max_nonpos's.
// Each branch holds its whole step, the four lines from u to a_t included.  They are the chain, and hipcc's schedule of it follows how
// they are written: shared behind the branches (a helper, a lambda, or variables declared in front) the same operations came out
// with the compare results in SGPR pairs instead of vcc and more wait states - 16.36 against 15.72 ms on the 786 455-position corpus
// at a switch cost, 42.00 against 41.59 ms with a matrix.  Written like this the listings are those of two separate kernels.
template <bool ONE_ROW, bool TRANS>
__global__ __launch_bounds__(kViterbiThreads) void viterbi_forward_kernel(const float *__restrict__ logits, int N, int C,
                                                                          const int32_t *__restrict__ rows, int M,
                                                                          const int32_t *__restrict__ vid_first,
                                                                          const int32_t *__restrict__ vid_count, float neg_cost,
                                                                          const float *__restrict__ trans, unsigned long long *__restrict__ stay,
                                                                          uint8_t *__restrict__ back, uint8_t *__restrict__ amax) {
  constexpr int P = TRANS ? trans_pitch<ONE_ROW>() : 1;                       // (without the matrix nothing of it exists: no tc, no sb)
  __shared__ float se[2][kViterbiTile][kEventMaxClasses];
  __shared__ __attribute__((aligned(16))) uint8_t sb[TRANS ? kViterbiTile : 1][kEventMaxClasses];      // b_t of the tile that is walked
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int V = *vid_count;
  float tc[P], t_stay = 0.f;
  if constexpr (TRANS) {
#pragma unroll
    for (int p = 0; p < P; ++p) tc[p] = (wave == 0 && p < C && lane < C) ? trans[p * C + lane] : -INFINITY;
    t_stay = (wave == 0 && lane < C) ? trans[lane * C + lane] : -INFINITY;
  }
  for (int vid = blockIdx.x; vid < V; vid += gridDim.x) {
    const video_span sp = video_of(vid_first, V, vid, M);
    const int vb = sp.vb, ve = sp.ve, ntiles = sp.ntiles;
    if (wave > 0) viterbi_stage<ONE_ROW>(se[0], vb, ve, logits, N, C, rows, wave, lane);
    __syncthreads();
    float v = 0.f;                                 // in front of position 0 every class scores 0: u_0 = e_0, whose maximum is 0
    for (int k = 0; k < ntiles; ++k) {
      const int t0 = vb + k * kViterbiTile;
      if (wave == 0) {
        const int n = min(kViterbiTile, ve - t0);
        const float(*buf)[kEventMaxClasses] = se[k & 1];
        unsigned long long my_stay = 0;
        int my_a = 0;
        // kViterbiChunk rows of e are read ahead of the chunk that is walked, so that no LDS latency sits on the chain.  The last
        // chunk of a video may run past position n - 1 on rows nobody staged: those steps reach no global store and v is not used
        // after them.
        float e[kViterbiChunk], e_next[kViterbiChunk];
#pragma unroll
        for (int i = 0; i < kViterbiChunk; ++i) e[i] = buf[i][lane];
        for (int j0 = 0; j0 < n; j0 += kViterbiChunk) {
#pragma unroll
          for (int i = 0; i < kViterbiChunk; ++i) e_next[i] = buf[min(j0 + kViterbiChunk + i, kViterbiTile - 1)][lane];
#pragma unroll
          for (int i = 0; i < kViterbiChunk; ++i) {
            if constexpr (TRANS) {
              float best = lane_f32(v, 0) + tc[0];
              int from = 0;
#pragma unroll
              for (int p = 1; p < P; ++p) {
                const float cand = lane_f32(v, p) + tc[p];
                if (cand > best) {
                  best = cand;
                  from = p;
                }
              }
              if (v + t_stay >= best) from = lane;                            // (the maximum holds this sum: >= is ==)
              const float w = (i == 0 && j0 == 0 && k == 0) ? 0.f : best;     // a video's first position has no predecessor: u_0 = e_0
              const float u = e[i] + w;
              const float mx = wave_max_nonpos<ONE_ROW>(u);
              const unsigned long long hit = __ballot(u == mx);
              v = u - mx;
              const int a = hit ? min(__ffsll(hit) - 1, C - 1) : 0;           // (no hit: a NaN among the inputs)
              sb[j0 + i][lane] = (uint8_t)from;
              if (lane == j0 + i) my_a = a;
            } else {
              const unsigned long long st = __ballot(v >= neg_cost);
              const float u = e[i] + max_nonpos(v, neg_cost);
              const float mx = wave_max_nonpos<ONE_ROW>(u);
              const unsigned long long hit = __ballot(u == mx);
              v = u - mx;
              const int a = hit ? min(__ffsll(hit) - 1, C - 1) : 0;
              if (lane == j0 + i) {
                my_stay = st;
                my_a = a;
              }
            }
          }
#pragma unroll
          for (int i = 0; i < kViterbiChunk; ++i) e[i] = e_next[i];
        }
        if constexpr (TRANS) {
          __builtin_amdgcn_wave_barrier();                                    // the rows above are read below by other lanes of this wave
          if constexpr (ONE_ROW) {
            if (lane < n) *(uint4 *)(back + (size_t)(t0 + lane) * P) = *(const uint4 *)&sb[lane][0];
          } else {
#pragma unroll
            for (int i = 0; i < P / 16; ++i) {
              const int f = i * 64 + lane, row = f / (P / 16), part = f % (P / 16);
              if (row < n) *(uint4 *)(back + (size_t)(t0 + row) * P + part * 16) = *(const uint4 *)&sb[row][part * 16];
            }
          }
        } else {
          if (lane < n) stay[t0 + lane] = my_stay;
        }
        if (lane < n) amax[t0 + lane] = (uint8_t)my_a;
      } else if (k + 1 < ntiles) {
        viterbi_stage<ONE_ROW>(se[(k + 1) & 1], t0 + kViterbiTile, ve, logits, N, C, rows, wave, lane);
      }
      __syncthreads();
    }
  }
}

// One wave per video.  Lane j of a tile stands for position t = its first position + j and holds nx = stay_{t+1} and at = a_t, so that
// label[t] = nx[label[t+1]] ? label[t+1] : at.  nx is 0 at the video's last position (take a_t) and all ones past it (pass through).
__global__ __launch_bounds__(64) void viterbi_backtrack_kernel(const unsigned long long *__restrict__ stay, const uint8_t *__restrict__ amax, int M,
                                                               const int32_t *__restrict__ vid_first, const int32_t *__restrict__ vid_count,
                                                               int32_t *__restrict__ label) {
  const int lane = threadIdx.x;
  const int V = *vid_count;
  for (int vid = blockIdx.x; vid < V; vid += gridDim.x) {
    const video_span sp = video_of(vid_first, V, vid, M);
    const int vb = sp.vb, ve = sp.ve, ntiles = sp.ntiles;
    auto load = [&](int k, unsigned long long &nx, int &at) {
      const int t = vb + k * kViterbiTile + lane;
      nx = ~0ull;
      at = 0;
      if (t < ve) {
        nx = t + 1 < ve ? stay[t + 1] : 0ull;
        at = amax[t];
      }
    };
    unsigned long long nx;
    int at, cur = 0;
    load(ntiles - 1, nx, at);
    for (int k = ntiles - 1; k >= 0; --k) {
      unsigned long long nx_front = ~0ull;
      int at_front = 0;
      if (k > 0) load(k - 1, nx_front, at_front);                              // in flight while this tile is walked
      const int nlo = (int)(unsigned)nx, nhi = (int)(unsigned)(nx >> 32);
      int my_label = 0;
#pragma unroll
      for (int j = kViterbiTile - 1; j >= 0; --j) {
        const unsigned long long mask = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(nhi, j) << 32) |
                                        (unsigned)__builtin_amdgcn_readlane(nlo, j);
        const int a = __builtin_amdgcn_readlane(at, j);
        cur = ((mask >> cur) & 1ull) ? cur : a;
        if (lane == j) my_label = cur;
      }
      const int t = vb + k * kViterbiTile + lane;
      if (t < ve) label[t] = my_label;
      nx = nx_front;
      at = at_front;
    }
  }
}

// One wave per video, tiles back to front.  Slot j of the LDS holds b_{t+1}, t = the tile's first position + j, so that
// label[t] = slot j [label[t+1]]: one dependent byte read per position.  The rows of the tile in front are loaded before the walk and
// stored into the LDS after it.  A byte is masked into the row, so that no read leaves the LDS whatever the workspace holds.
template <bool ONE_ROW>
__global__ __launch_bounds__(64) void viterbi_trans_backtrack_kernel(const uint8_t *__restrict__ back, const uint8_t *__restrict__ amax, int M,
                                                                     const int32_t *__restrict__ vid_first,
                                                                     const int32_t *__restrict__ vid_count, int32_t *__restrict__ label) {
  constexpr int P = trans_pitch<ONE_ROW>(), Q = P / 16;                       // Q: 16-byte parts of a row
  __shared__ __attribute__((aligned(16))) uint8_t sb[kViterbiTile * P];
  const int lane = threadIdx.x;
  const int V = *vid_count;
  for (int vid = blockIdx.x; vid < V; vid += gridDim.x) {
    const video_span sp = video_of(vid_first, V, vid, M);
    const int vb = sp.vb, ve = sp.ve, ntiles = sp.ntiles;
    uint4 part[Q];
    auto load = [&](int k) {                                                  // the rows of positions first + 1 .. first + kViterbiTile
      const int t1 = vb + k * kViterbiTile + 1;
#pragma unroll
      for (int i = 0; i < Q; ++i) {
        const int f = i * 64 + lane, t = t1 + f / Q;
        part[i] = make_uint4(0, 0, 0, 0);
        if (t < ve) part[i] = ((const uint4 *)(back + (size_t)t * P))[f % Q];
      }
    };
    auto put = [&]() {
#pragma unroll
      for (int i = 0; i < Q; ++i) ((uint4 *)sb)[i * 64 + lane] = part[i];
    };
    load(ntiles - 1);
    put();
    __syncthreads();
    int cur = amax[ve - 1] & (P - 1);
    for (int k = ntiles - 1; k >= 0; --k) {
      if (k > 0) load(k - 1);                                                  // in flight while this tile is walked
      const int t0 = vb + k * kViterbiTile, n = min(kViterbiTile, ve - t0);
      int my_label = 0, j = n - 1;
      if (k == ntiles - 1) {                                                   // the video's last position takes a_t
        if (lane == j) my_label = cur;
        --j;
      }
#pragma unroll 4
      for (; j >= 0; --j) {
        cur = sb[j * P + cur] & (P - 1);
        if (lane == j) my_label = cur;
      }
      if (lane < n) label[t0 + lane] = my_label;
      __syncthreads();
      if (k > 0) {
        put();
        __syncthreads();
      }
    }
  }
}

// One thread per position, one workgroup per tile of kEventTile: flags and tile counts for the scan and scatter above.
//   PATH = false  flags[m] = a video begins at m: scan and scatter then list the videos' first positions
//   PATH = true   flags[m] = a run of `label` begins at m, and conf[m] = softmax(q)[label[m]] with event_score_kernel's operations
template <bool PATH>
__global__ __launch_bounds__(kEventTile) void event_flag_kernel(const float *__restrict__ logits, int N, int C, const int32_t *__restrict__ rows,
                                                                const int32_t *__restrict__ start, int M, const int32_t *__restrict__ label,
                                                                float *__restrict__ conf, uint8_t *__restrict__ flags,
                                                                int32_t *__restrict__ counts) {
  __shared__ int wcnt[kEventTile / 64];
  const int tid = threadIdx.x, m = blockIdx.x * kEventTile + tid;
  int f = 0;
  if (m < M) {
    f = (m == 0 || start[m] != 0) ? 1 : 0;
    if constexpr (PATH) {
      const int lab = label[m];
      if (!f) f = label[m - 1] != lab ? 1 : 0;
      const float *q = logits + (size_t)min(max(rows[m], 0), N - 1) * C;
      float mx = q[0];
      for (int c = 1; c < C; ++c) mx = fmaxf(mx, q[c]);
      float sum = 0.f, el = 0.f;
      for (int c = 0; c < C; ++c) {
        const float e = expf(q[c] - mx);
        sum += e;
        if (c == lab) el = e;
      }
      conf[m] = el / sum;
    }
    flags[m] = (uint8_t)f;
  }
  const int nw = __popcll(__ballot(f));
  if ((tid & 63) == 0) wcnt[tid >> 6] = nw;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int k = 0; k < kEventTile / 64; ++k) total += wcnt[k];
    counts[blockIdx.x] = total;
  }
}

// ---- posteriors under the transition matrix: forward-backward in the log domain ----

constexpr float kLog2e = 1.44269504088896340736f, kLn2 = 0.69314718055994530942f;

// One direction of the recurrence over every chain this workgroup takes.  Lane l holds element l of the running vector and tm, its slice
// of the matrix: the column T[:, l] forward (the sum runs over the predecessors p), the row T[l, :] backward (over the successors c);
// -inf past C, so that a lane or a term past C is -inf throughout.  x is the vector a step reads through readlane:
//   forward   x = ah_{t-1};           r[c] = LSE_p(x[p] + T[p, c]);  a_t = e_t + r;  ah_t = a_t - max a_t          -> out[t]
//   backward  x = e_{t+1} + bh_{t+1};  r[p] = LSE_c(T[p, c] + x[c]);  bh_t = r - max r                              -> out[t]
// Every candidate is <= 0 or -inf (ah, bh, e, T <= 0), so their maximum is max_nonpos's; r itself may pass 0 (by at most ln C).  A
// column whose candidates are all -inf gives -inf: its maximum is replaced by 0, the sum is 0 and its logarithm -inf.  The finite
// diagonal keeps every b_t[p] and at least one a_t[c] finite, so the wave maximum is finite and no value is NaN.
// The C exponentials of a step are v_exp_f32 on (x - mx) log2(e) and the logarithm v_log_f32 times ln 2: each is within an ulp or two
// of its argument's rounding, and the terms that count have |x - mx| < 17, where that rounding is below the sum's own.
// A step past the chain's last position (the read-ahead works in whole chunks) is skipped as a whole: backward the short tile is
// walked first, so x must not move there.
template <bool ONE_ROW, bool BACKWARD>
__device__ __forceinline__ void hmm_chain(float (*se)[kViterbiTile][kEventMaxClasses], const float *__restrict__ logits, int N, int C,
                                          const int32_t *__restrict__ rows, int M, const int32_t *__restrict__ vid_first, int V,
                                          const float *__restrict__ trans, float *__restrict__ out) {
  constexpr int P = trans_pitch<ONE_ROW>();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float tm[P];
#pragma unroll
  for (int i = 0; i < P; ++i) tm[i] = (wave == 0 && i < C && lane < C) ? trans[BACKWARD ? lane * C + i : i * C + lane] : -INFINITY;
  const float open = lane < C ? 0.f : -INFINITY;   // r of a chain's first step: no predecessor forward (a_0 = e_0), b_{L-1} = 0 backward
  for (int ch = blockIdx.x; ch < 2 * V; ch += gridDim.x) {                    // (the grid is even: a workgroup keeps its direction)
    const video_span sp = video_of(vid_first, V, ch >> 1, M);
    const int vb = sp.vb, ve = sp.ve, ntiles = sp.ntiles;
    if (wave > 0) viterbi_stage<ONE_ROW>(se[0], vb + (BACKWARD ? ntiles - 1 : 0) * kViterbiTile, ve, logits, N, C, rows, wave, lane);
    __syncthreads();
    float x = open;
    for (int k = 0; k < ntiles; ++k) {
      const int t0 = vb + (BACKWARD ? ntiles - 1 - k : k) * kViterbiTile;
      if (wave == 0) {
        const int n = min(kViterbiTile, ve - t0);
        const float(*buf)[kEventMaxClasses] = se[k & 1];
        // step s of a tile takes its row s forward and n - 1 - s backward; kViterbiChunk rows are read ahead of the chain
        float e[kViterbiChunk], e_next[kViterbiChunk];
#pragma unroll
        for (int i = 0; i < kViterbiChunk; ++i) e[i] = buf[BACKWARD ? max(n - 1 - i, 0) : i][lane];
        for (int j0 = 0; j0 < n; j0 += kViterbiChunk) {
#pragma unroll
          for (int i = 0; i < kViterbiChunk; ++i) {
            const int s = j0 + kViterbiChunk + i;
            e_next[i] = buf[BACKWARD ? max(n - 1 - s, 0) : min(s, kViterbiTile - 1)][lane];
          }
#pragma unroll
          for (int i = 0; i < kViterbiChunk; ++i) {
            const int s = j0 + i;
            if (s < n) {                                                      // (wave-uniform)
              float cand[P];
#pragma unroll
              for (int p = 0; p < P; ++p) cand[p] = lane_f32(x, p) + tm[p];
              float mx = cand[0];
#pragma unroll
              for (int p = 1; p < P; ++p) mx = max_nonpos(mx, cand[p]);
              if (mx == -INFINITY) mx = 0.f;
              float sum = 0.f;
#pragma unroll
              for (int p = 0; p < P; ++p) sum += __builtin_amdgcn_exp2f((cand[p] - mx) * kLog2e);
              const float r = (s == 0 && k == 0) ? open : mx + __builtin_amdgcn_logf(sum) * kLn2;
              float keep;
              if constexpr (BACKWARD) {
                keep = r - wave_max<ONE_ROW>(r);
                x = e[i] + keep;
              } else {
                const float a = e[i] + r;
                keep = a - wave_max<ONE_ROW>(a);
                x = keep;
              }
              if (lane < P) out[(size_t)(t0 + (BACKWARD ? n - 1 - s : s)) * P + lane] = keep;
            }
          }
#pragma unroll
          for (int i = 0; i < kViterbiChunk; ++i) e[i] = e_next[i];
        }
      } else if (k + 1 < ntiles) {
        viterbi_stage<ONE_ROW>(se[(k + 1) & 1], BACKWARD ? t0 - kViterbiTile : t0 + kViterbiTile, ve, logits, N, C, rows, wave, lane);
      }
      __syncthreads();
    }
  }
}

// chain 2 v walks video v forward into fwd, chain 2 v + 1 walks it backward into bwd: rows of trans_pitch floats per position
template <bool ONE_ROW>
__global__ __launch_bounds__(kViterbiThreads) void hmm_chain_kernel(const float *__restrict__ logits, int N, int C, const int32_t *__restrict__ rows,
                                                                    int M, const int32_t *__restrict__ vid_first,
                                                                    const int32_t *__restrict__ vid_count, const float *__restrict__ trans,
                                                                    float *__restrict__ fwd, float *__restrict__ bwd) {
  __shared__ float se[2][kViterbiTile][kEventMaxClasses];
  const int V = *vid_count;
  if (blockIdx.x & 1)
    hmm_chain<ONE_ROW, true>(se, logits, N, C, rows, M, vid_first, V, trans, bwd);
  else
    hmm_chain<ONE_ROW, false>(se, logits, N, C, rows, M, vid_first, V, trans, fwd);
}

// One thread per position: gamma = softmax(ah + bh) - maximum subtracted, accurate expf, the sum in ascending c, one division per
// value - into posterior (M, C) if there is one, and conf[m] = gamma[label[m]], the value that is stored.
template <bool ONE_ROW>
__global__ __launch_bounds__(kEventThreads) void hmm_posterior_kernel(const float *__restrict__ fwd, const float *__restrict__ bwd, int C, int M,
                                                                      const int32_t *__restrict__ label, float *__restrict__ posterior,
                                                                      float *__restrict__ conf) {
  constexpr int P = trans_pitch<ONE_ROW>();
  const int m = blockIdx.x * kEventThreads + threadIdx.x;
  if (m >= M) return;
  const float *a = fwd + (size_t)m * P, *b = bwd + (size_t)m * P;
  float mx = a[0] + b[0];
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, a[c] + b[c]);
  float sum = 0.f;
  for (int c = 0; c < C; ++c) sum += expf(a[c] + b[c] - mx);
  const int lab = label[m];
  float mine = 0.f;
  for (int c = 0; c < C; ++c) {
    const float g = expf(a[c] + b[c] - mx) / sum;
    if (posterior) posterior[(size_t)m * C + c] = g;
    if (c == lab) mine = g;
  }
  conf[m] = mine;
}

}  // namespace

// what either chain keeps between its launches: the tail of its workspace, behind what the path itself stores per position
struct event_chain {
  void *ws;
  size_t bytes;
  int32_t *vid_first;      //   [max_positions]   the first position of every video
  int32_t *vid_count;      //   [1]
  uint8_t *amax;           //   [max_positions]   a_t
};

struct tn_event_decoder {
  tn_ctx *ctx;
  int max_positions, max_classes, max_tiles;
  void *ws;                // one allocation:
  int32_t *label;          //   [max_positions]   used where the caller passes no label_out
  float *conf;             //   [max_positions]   ... no conf_out
  int32_t *counts, *offsets;   // [max_tiles] each
  uint8_t *flags;          //   [max_positions]
  size_t ws_bytes;
  event_chain path;        // the switch-cost path's, allocated by the first tn_event_decoder_run_switch, in front of the chain's:
  unsigned long long *stay;    // [max_positions]   bit c: v_{t-1}[c] >= -cost
  event_chain trans;       // the transition-matrix path's, allocated by the first tn_event_decoder_run_transitions, in front:
  uint8_t *back;           //   [max_positions][pitch]   b_t, pitch = 16 bytes for max_classes <= 16, else 64
  float *matrix;           //   [max_classes^2]   the call's matrix, (C, C) row-major
  float *post;             // allocated by the first tn_event_decoder_run_posteriors: [2][max_positions][pitch] fp32, ah_t and then bh_t,
  size_t post_bytes;       //   pitch = 16 floats for max_classes <= 16, else 64
};

namespace {

struct event_in {
  const float *logits;
  int N, C;
  const int32_t *rows, *start;
  int M;
};

struct event_out {
  int32_t *label;          // the caller's or the handle's
  float *conf;
  int32_t *first, *last, *cls;
  float *score, *peak;
  int32_t *count;
};

size_t padded_positions(const tn_event_decoder *d) { return ((size_t)d->max_positions + 3) & ~(size_t)3; }

// The checks the three entries share, in the one order they are made in.  own_null: the entry's own pointer argument is null (the
// message, checked behind start); own_bad: the entry's own parameter is refused (the message, checked behind C); nullptr: neither.
int check_run(const char *entry, const tn_event_decoder *d, const event_in &in, const char *own_null, const char *own_bad, const event_out &out) {
  const std::string fn = std::string(entry) + ": ";
  TN_REQUIRE(d, fn + "null handle");
  TN_REQUIRE(in.logits, fn + "logits is null");
  TN_REQUIRE(in.rows, fn + "rows is null");
  TN_REQUIRE(in.start, fn + "start is null");
  TN_REQUIRE(!own_null, fn + own_null);
  TN_REQUIRE(out.first, fn + "ev_first is null");
  TN_REQUIRE(out.last, fn + "ev_last is null");
  TN_REQUIRE(out.cls, fn + "ev_cls is null");
  TN_REQUIRE(out.score, fn + "ev_score is null");
  TN_REQUIRE(out.peak, fn + "ev_peak is null");
  TN_REQUIRE(out.count, fn + "count is null");
  TN_REQUIRE(in.N >= 1, fn + "N must be >= 1");
  TN_REQUIRE(in.C >= 1 && in.C <= kEventMaxClasses, fn + "C must be in [1, 64]");
  TN_REQUIRE(in.C <= d->max_classes, fn + "C exceeds the handle's max_classes");
  TN_REQUIRE(!own_bad, fn + own_bad);
  TN_REQUIRE(in.M >= 1, fn + "M must be >= 1");
  TN_REQUIRE(in.M <= d->max_positions, fn + "M exceeds the handle's max_positions");
  return TN_OK;
}

// label_out / conf_out NULL: the handle's own buffers
void own_frames(const tn_event_decoder *d, event_out &out) {
  if (!out.label) out.label = d->label;
  if (!out.conf) out.conf = d->conf;
}

int event_tiles(int M) { return (M + kEventTile - 1) / kEventTile; }

// the positions of the set flags, in order -> first; their number -> *count
void list_flags(tn_event_decoder *d, hipStream_t s, int M, int32_t *count, int32_t *first) {
  const int tiles = event_tiles(M);
  hipLaunchKernelGGL(event_scan_kernel, dim3(1), dim3(kEventScanBlock), 0, s, d->counts, tiles, d->offsets, count);
  hipLaunchKernelGGL(event_scatter_kernel, dim3(tiles), dim3(kEventTile), 0, s, d->flags, M, d->offsets, first);
}

// the videos' first positions: the set flags of start through the scan and scatter of the runs
void find_videos(tn_event_decoder *d, hipStream_t s, const event_in &in, const event_chain &c) {
  hipLaunchKernelGGL(event_flag_kernel<false>, dim3(event_tiles(in.M)), dim3(kEventTile), 0, s, in.logits, in.N, in.C, in.rows, in.start, in.M,
                     (const int32_t *)nullptr, (float *)nullptr, d->flags, d->counts);
  list_flags(d, s, in.M, c.vid_count, c.vid_first);
}

// label, conf and the run-start flags with their tile counts -> the events
void reduce_events(tn_event_decoder *d, hipStream_t s, int M, const event_out &out) {
  list_flags(d, s, M, out.count, out.first);
  const int blocks = std::min((M + 3) / 4, 2048);
  hipLaunchKernelGGL(event_reduce_kernel, dim3(blocks), dim3(256), 0, s, out.label, out.conf, M, out.count, out.first, out.last, out.cls,
                     out.score, out.peak);
}

// a label path -> conf and the events
void emit_events(tn_event_decoder *d, hipStream_t s, const event_in &in, const event_out &out) {
  hipLaunchKernelGGL(event_flag_kernel<true>, dim3(event_tiles(in.M)), dim3(kEventTile), 0, s, in.logits, in.N, in.C, in.rows, in.start, in.M,
                     out.label, out.conf, d->flags, d->counts);
  reduce_events(d, s, in.M, out);
}

// A path's workspace, allocated by the first call that needs it: `own` bytes of the path's (a multiple of 4) and then the chain's.
int chain_workspace(const tn_event_decoder *d, event_chain &c, size_t own, const char *entry, const char *what) {
  if (c.ws) return TN_OK;
  const size_t mp = padded_positions(d), bytes = own + mp * (4 + 1) + 4;
  void *ws = nullptr;
  if (hipMalloc(&ws, bytes) != hipSuccess) {
    (void)hipGetLastError();
    tn_set_error(std::string(entry) + ": device allocation of the " + what + " workspace failed (" + std::to_string(bytes) + " bytes)");
    return TN_ERR_NOMEM;
  }
  c.ws = ws;
  c.bytes = bytes;
  c.vid_first = (int32_t *)((char *)ws + own);
  c.vid_count = c.vid_first + mp;
  c.amax = (uint8_t *)(c.vid_count + 1);
  return TN_OK;
}

template <bool ONE_ROW, bool TRANS>
void launch_forward(const tn_event_decoder *d, hipStream_t s, const event_in &in, const event_chain &c, int chains, float neg_cost) {
  hipLaunchKernelGGL((viterbi_forward_kernel<ONE_ROW, TRANS>), dim3(chains), dim3(kViterbiThreads), 0, s, in.logits, in.N, in.C, in.rows, in.M,
                     c.vid_first, c.vid_count, neg_cost, TRANS ? d->matrix : nullptr, TRANS ? nullptr : d->stay, TRANS ? d->back : nullptr,
                     c.amax);
}

}  // namespace

extern "C" int tn_event_decoder_create(tn_ctx *ctx, int max_positions, int max_classes, tn_event_decoder **out) {
  TN_REQUIRE(ctx && out, "tn_event_decoder_create: null argument (ctx, out)");
  TN_REQUIRE(max_positions >= 1 && max_positions <= (1 << 30), "tn_event_decoder_create: max_positions must be in [1, 2^30]");
  TN_REQUIRE(max_classes >= 1 && max_classes <= 64, "tn_event_decoder_create: max_classes must be in [1, 64]");
  TN_ON_DEVICE(ctx->device);
  tn_event_decoder *d = new tn_event_decoder();
  d->ctx = ctx;
  d->max_positions = max_positions;
  d->max_classes = max_classes;
  d->max_tiles = event_tiles(max_positions);
  const size_t mp = padded_positions(d), mt = d->max_tiles;
  d->ws_bytes = mp * 4 * 2 + mt * 4 * 2 + mp;
  if (hipMalloc(&d->ws, d->ws_bytes) != hipSuccess) {
    delete d;
    tn_set_error("device allocation failed");
    return TN_ERR_NOMEM;
  }
  d->label = (int32_t *)d->ws;
  d->conf = (float *)(d->label + mp);
  d->counts = (int32_t *)(d->conf + mp);
  d->offsets = d->counts + mt;
  d->flags = (uint8_t *)(d->offsets + mt);
  *out = d;
  return TN_OK;
}

extern "C" int tn_event_decoder_destroy(tn_event_decoder *d) {
  if (!d) return TN_OK;
  TnDeviceGuard tn_dg_(d->ctx->device);
  (void)hipStreamSynchronize(d->ctx->stream);
  (void)hipFree(d->ws);
  if (d->path.ws) (void)hipFree(d->path.ws);
  if (d->trans.ws) (void)hipFree(d->trans.ws);
  if (d->post) (void)hipFree(d->post);
  delete d;
  return TN_OK;
}

extern "C" int tn_event_decoder_run(tn_event_decoder *d, const float *logits, int N, int C, const int32_t *rows, const int32_t *start, int M,
                                    int width, int32_t *label_out, float *conf_out, int32_t *ev_first, int32_t *ev_last, int32_t *ev_cls,
                                    float *ev_score, float *ev_peak, int32_t *count, void *stream) {
  const event_in in{logits, N, C, rows, start, M};
  event_out out{label_out, conf_out, ev_first, ev_last, ev_cls, ev_score, ev_peak, count};
  const char *bad = !(width >= 1 && width <= 63) ? "width must be in [1, 63]" : width % 2 != 1 ? "width must be odd" : nullptr;
  if (const int rc = check_run("tn_event_decoder_run", d, in, nullptr, bad, out)) return rc;
  TN_ON_DEVICE(d->ctx->device);
  hipStream_t s = stream ? (hipStream_t)stream : d->ctx->stream;
  own_frames(d, out);
  const int h = (width - 1) / 2, tiles = event_tiles(M);
  const size_t lds = event_lds_bytes(C, h);
  if (C % 4 == 0 && ((uintptr_t)logits & 15) == 0)
    hipLaunchKernelGGL(event_score_kernel<true>, dim3(tiles), dim3(kEventThreads), lds, s, logits, N, C, rows, start, M, h, out.label, out.conf,
                       d->flags, d->counts);
  else
    hipLaunchKernelGGL(event_score_kernel<false>, dim3(tiles), dim3(kEventThreads), lds, s, logits, N, C, rows, start, M, h, out.label, out.conf,
                       d->flags, d->counts);
  reduce_events(d, s, M, out);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

extern "C" int tn_dbg_event_decoder_geometry(int *tile, int *scan_block) {
  TN_REQUIRE(tile && scan_block, "tn_dbg_event_decoder_geometry: null argument (tile, scan_block)");
  *tile = kEventTile;
  *scan_block = kEventScanBlock;
  return TN_OK;
}

extern "C" int tn_event_decoder_run_switch(tn_event_decoder *d, const float *logits, int N, int C, const int32_t *rows, const int32_t *start,
                                           int M, float switch_cost, int32_t *label_out, float *conf_out, int32_t *ev_first, int32_t *ev_last,
                                           int32_t *ev_cls, float *ev_score, float *ev_peak, int32_t *count, void *stream) {
  const char *entry = "tn_event_decoder_run_switch";
  const event_in in{logits, N, C, rows, start, M};
  event_out out{label_out, conf_out, ev_first, ev_last, ev_cls, ev_score, ev_peak, count};
  const char *bad = std::isfinite(switch_cost) && switch_cost >= 0.f ? nullptr : "switch_cost must be finite and >= 0";
  if (const int rc = check_run(entry, d, in, nullptr, bad, out)) return rc;
  TN_ON_DEVICE(d->ctx->device);
  if (const int rc = chain_workspace(d, d->path, padded_positions(d) * 8, entry, "path")) return rc;
  d->stay = (unsigned long long *)d->path.ws;
  hipStream_t s = stream ? (hipStream_t)stream : d->ctx->stream;
  own_frames(d, out);
  find_videos(d, s, in, d->path);
  const int chains = std::min(M, kViterbiMaxGrid);
  if (C <= 16)
    launch_forward<true, false>(d, s, in, d->path, chains, -switch_cost);
  else
    launch_forward<false, false>(d, s, in, d->path, chains, -switch_cost);
  hipLaunchKernelGGL(viterbi_backtrack_kernel, dim3(chains), dim3(64), 0, s, d->stay, d->path.amax, M, d->path.vid_first, d->path.vid_count,
                     out.label);
  emit_events(d, s, in, out);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

extern "C" int tn_dbg_event_decoder_switch_geometry(int *tile) {
  TN_REQUIRE(tile, "tn_dbg_event_decoder_switch_geometry: null argument (tile)");
  *tile = kViterbiTile;
  return TN_OK;
}

namespace {

// The path under the matrix, and with `posteriors` the marginals under it: conf is then gamma's and `posterior` (may be null) takes gamma.
int run_matrix(const char *entry, tn_event_decoder *d, const event_in &in, const float *transitions, event_out out, bool posteriors,
               float *posterior, void *stream) {
  const int C = in.C, M = in.M;
  if (const int rc = check_run(entry, d, in, transitions ? nullptr : "transitions is null", nullptr, out)) return rc;
  for (int p = 0; p < C; ++p)
    for (int c = 0; c < C; ++c) {
      const float x = transitions[p * C + c];
      const char *why = std::isnan(x) ? "is NaN" : x > 0.f ? "is positive: a transition score must be <= 0 or -inf"
                        : (p == c && std::isinf(x)) ? "is not finite: staying must always be possible" : nullptr;
      if (why) {
        tn_set_error(std::string(entry) + ": transitions[" + std::to_string(p) + "][" + std::to_string(c) + "] " + why);
        return TN_ERR_INVALID;
      }
    }
  TN_ON_DEVICE(d->ctx->device);
  const bool one_row = d->max_classes <= 16;                // (the pitch of the workspace follows the handle, not the call)
  const size_t pitch = one_row ? trans_pitch<true>() : trans_pitch<false>(), rows_bytes = padded_positions(d) * pitch;
  if (const int rc = chain_workspace(d, d->trans, rows_bytes + (size_t)d->max_classes * d->max_classes * 4, entry, "back-pointer")) return rc;
  d->back = (uint8_t *)d->trans.ws;
  d->matrix = (float *)(d->back + rows_bytes);
  const size_t post_half = (size_t)d->max_positions * pitch;                 // floats of ah, and of bh behind it
  if (posteriors && !d->post) {
    const size_t bytes = 2 * post_half * 4;
    void *ws = nullptr;
    if (hipMalloc(&ws, bytes) != hipSuccess) {
      (void)hipGetLastError();
      tn_set_error(std::string(entry) + ": device allocation of the posterior workspace failed (" + std::to_string(bytes) + " bytes)");
      return TN_ERR_NOMEM;
    }
    d->post = (float *)ws;
    d->post_bytes = bytes;
  }
  hipStream_t s = stream ? (hipStream_t)stream : d->ctx->stream;
  TN_HIP_CHECK(hipMemcpyAsync(d->matrix, transitions, (size_t)C * C * 4, hipMemcpyHostToDevice, s));
  own_frames(d, out);
  find_videos(d, s, in, d->trans);
  const int chains = std::min(M, kViterbiMaxGrid);
  if (one_row) {
    launch_forward<true, true>(d, s, in, d->trans, chains, 0.f);
    hipLaunchKernelGGL(viterbi_trans_backtrack_kernel<true>, dim3(chains), dim3(64), 0, s, d->back, d->trans.amax, M, d->trans.vid_first,
                       d->trans.vid_count, out.label);
  } else {
    launch_forward<false, true>(d, s, in, d->trans, chains, 0.f);
    hipLaunchKernelGGL(viterbi_trans_backtrack_kernel<false>, dim3(chains), dim3(64), 0, s, d->back, d->trans.amax, M, d->trans.vid_first,
                       d->trans.vid_count, out.label);
  }
  if (!posteriors) {
    emit_events(d, s, in, out);
  } else {
    static_assert(kViterbiMaxGrid % 2 == 0, "a workgroup of the chain kernel keeps its direction");
    const int both = (int)std::min<long long>(2ll * M, kViterbiMaxGrid), blocks = (M + kEventThreads - 1) / kEventThreads;
    float *fwd = d->post, *bwd = d->post + post_half;
    hipLaunchKernelGGL(event_flag_kernel<true>, dim3(event_tiles(M)), dim3(kEventTile), 0, s, in.logits, in.N, C, in.rows, in.start, M,
                       out.label, out.conf, d->flags, d->counts);
    if (one_row) {
      hipLaunchKernelGGL(hmm_chain_kernel<true>, dim3(both), dim3(kViterbiThreads), 0, s, in.logits, in.N, C, in.rows, M, d->trans.vid_first,
                         d->trans.vid_count, d->matrix, fwd, bwd);
      hipLaunchKernelGGL(hmm_posterior_kernel<true>, dim3(blocks), dim3(kEventThreads), 0, s, fwd, bwd, C, M, out.label, posterior, out.conf);
    } else {
      hipLaunchKernelGGL(hmm_chain_kernel<false>, dim3(both), dim3(kViterbiThreads), 0, s, in.logits, in.N, C, in.rows, M, d->trans.vid_first,
                         d->trans.vid_count, d->matrix, fwd, bwd);
      hipLaunchKernelGGL(hmm_posterior_kernel<false>, dim3(blocks), dim3(kEventThreads), 0, s, fwd, bwd, C, M, out.label, posterior, out.conf);
    }
    reduce_events(d, s, M, out);
  }
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

}  // namespace

extern "C" int tn_event_decoder_run_transitions(tn_event_decoder *d, const float *logits, int N, int C, const int32_t *rows,
                                                const int32_t *start, int M, const float *transitions, int32_t *label_out,
                                                float *conf_out, int32_t *ev_first, int32_t *ev_last, int32_t *ev_cls, float *ev_score,
                                                float *ev_peak, int32_t *count, void *stream) {
  return run_matrix("tn_event_decoder_run_transitions", d, {logits, N, C, rows, start, M}, transitions,
                    {label_out, conf_out, ev_first, ev_last, ev_cls, ev_score, ev_peak, count}, false, nullptr, stream);
}

extern "C" int tn_event_decoder_run_posteriors(tn_event_decoder *d, const float *logits, int N, int C, const int32_t *rows,
                                               const int32_t *start, int M, const float *transitions, int32_t *label_out, float *conf_out,
                                               float *posterior, int32_t *ev_first, int32_t *ev_last, int32_t *ev_cls, float *ev_score,
                                               float *ev_peak, int32_t *count, void *stream) {
  return run_matrix("tn_event_decoder_run_posteriors", d, {logits, N, C, rows, start, M}, transitions,
                    {label_out, conf_out, ev_first, ev_last, ev_cls, ev_score, ev_peak, count}, true, posterior, stream);
}

extern "C" int tn_dbg_event_decoder_transition_geometry(int *tile, int *pitch16, int *pitch64) {
  TN_REQUIRE(tile && pitch16 && pitch64, "tn_dbg_event_decoder_transition_geometry: null argument (tile, pitch16, pitch64)");
  *tile = kViterbiTile;
  *pitch16 = trans_pitch<true>();
  *pitch64 = trans_pitch<false>();
  return TN_OK;
}

extern "C" int tn_dbg_event_decoder_workspace_bytes(const tn_event_decoder *d, size_t *bytes) {
  TN_REQUIRE(d && bytes, "tn_dbg_event_decoder_workspace_bytes: null argument (handle, bytes)");
  *bytes = d->ws_bytes + d->path.bytes + d->trans.bytes + d->post_bytes;
  return TN_OK;
}
