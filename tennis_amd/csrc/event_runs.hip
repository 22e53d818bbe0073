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
#include "common.h"

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

}  // namespace

struct tn_event_decoder {
  tn_ctx *ctx;
  int max_positions, max_classes, max_tiles;
  void *ws;                // one allocation:
  int32_t *label;          //   [max_positions]   used where the caller passes no label_out
  float *conf;             //   [max_positions]   ... no conf_out
  int32_t *counts, *offsets;   // [max_tiles] each
  uint8_t *flags;          //   [max_positions]
};

extern "C" int tn_event_decoder_create(tn_ctx *ctx, int max_positions, int max_classes, tn_event_decoder **out) {
  TN_REQUIRE(ctx && out, "tn_event_decoder_create: null argument (ctx, out)");
  TN_REQUIRE(max_positions >= 1 && max_positions <= (1 << 30), "tn_event_decoder_create: max_positions must be in [1, 2^30]");
  TN_REQUIRE(max_classes >= 1 && max_classes <= 64, "tn_event_decoder_create: max_classes must be in [1, 64]");
  TN_ON_DEVICE(ctx->device);
  tn_event_decoder *d = new tn_event_decoder();
  d->ctx = ctx;
  d->max_positions = max_positions;
  d->max_classes = max_classes;
  d->max_tiles = (max_positions + kEventTile - 1) / kEventTile;
  const size_t mp = ((size_t)max_positions + 3) & ~(size_t)3, mt = d->max_tiles;
  if (hipMalloc(&d->ws, mp * 4 * 2 + mt * 4 * 2 + mp) != hipSuccess) {
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
  delete d;
  return TN_OK;
}

extern "C" int tn_event_decoder_run(tn_event_decoder *d, const float *logits, int N, int C, const int32_t *rows, const int32_t *start, int M,
                                    int width, int32_t *label_out, float *conf_out, int32_t *ev_first, int32_t *ev_last, int32_t *ev_cls,
                                    float *ev_score, float *ev_peak, int32_t *count, void *stream) {
  TN_REQUIRE(d, "tn_event_decoder_run: null handle");
  TN_REQUIRE(logits, "tn_event_decoder_run: logits is null");
  TN_REQUIRE(rows, "tn_event_decoder_run: rows is null");
  TN_REQUIRE(start, "tn_event_decoder_run: start is null");
  TN_REQUIRE(ev_first, "tn_event_decoder_run: ev_first is null");
  TN_REQUIRE(ev_last, "tn_event_decoder_run: ev_last is null");
  TN_REQUIRE(ev_cls, "tn_event_decoder_run: ev_cls is null");
  TN_REQUIRE(ev_score, "tn_event_decoder_run: ev_score is null");
  TN_REQUIRE(ev_peak, "tn_event_decoder_run: ev_peak is null");
  TN_REQUIRE(count, "tn_event_decoder_run: count is null");
  TN_REQUIRE(N >= 1, "tn_event_decoder_run: N must be >= 1");
  TN_REQUIRE(C >= 1 && C <= 64, "tn_event_decoder_run: C must be in [1, 64]");
  TN_REQUIRE(C <= d->max_classes, "tn_event_decoder_run: C exceeds the handle's max_classes");
  TN_REQUIRE(width >= 1 && width <= 63, "tn_event_decoder_run: width must be in [1, 63]");
  TN_REQUIRE(width % 2 == 1, "tn_event_decoder_run: width must be odd");
  TN_REQUIRE(M >= 1, "tn_event_decoder_run: M must be >= 1");
  TN_REQUIRE(M <= d->max_positions, "tn_event_decoder_run: M exceeds the handle's max_positions");
  TN_ON_DEVICE(d->ctx->device);
  hipStream_t s = stream ? (hipStream_t)stream : d->ctx->stream;
  const int h = (width - 1) / 2, tiles = (M + kEventTile - 1) / kEventTile;
  int32_t *label = label_out ? label_out : d->label;
  float *conf = conf_out ? conf_out : d->conf;
  const size_t lds = event_lds_bytes(C, h);
  if (C % 4 == 0 && ((uintptr_t)logits & 15) == 0)
    hipLaunchKernelGGL(event_score_kernel<true>, dim3(tiles), dim3(kEventThreads), lds, s, logits, N, C, rows, start, M, h, label, conf,
                       d->flags, d->counts);
  else
    hipLaunchKernelGGL(event_score_kernel<false>, dim3(tiles), dim3(kEventThreads), lds, s, logits, N, C, rows, start, M, h, label, conf,
                       d->flags, d->counts);
  hipLaunchKernelGGL(event_scan_kernel, dim3(1), dim3(kEventScanBlock), 0, s, d->counts, tiles, d->offsets, count);
  hipLaunchKernelGGL(event_scatter_kernel, dim3(tiles), dim3(kEventTile), 0, s, d->flags, M, d->offsets, ev_first);
  const int blocks = std::min((M + 3) / 4, 2048);
  hipLaunchKernelGGL(event_reduce_kernel, dim3(blocks), dim3(256), 0, s, label, conf, M, count, ev_first, ev_last, ev_cls, ev_score, ev_peak);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

extern "C" int tn_dbg_event_decoder_geometry(int *tile, int *scan_block) {
  TN_REQUIRE(tile && scan_block, "tn_dbg_event_decoder_geometry: null argument (tile, scan_block)");
  *tile = kEventTile;
  *scan_block = kEventScanBlock;
  return TN_OK;
}
