// Temporal activation maps of the windowed heads (CNNRNN / TemporalPooling(max), models/vision/definitions.py:66-69,106-109: both end
// in max over T -> Dense).  With step[b][k] the window position the pool read unit k from,
//   logit[b][c] = bias[c] + sum_k W[c][k] * pooled[b][k] = bias[c] + sum_t tam[b][c][t],
//   tam[b][c][t] = sum over { k : step[b][k] == t } of W[c][k] * pooled[b][k]
// - the Dense's sum regrouped by the step each term was read from; no backward pass.  The reference has no counterpart.
//
// The straightforward form: a workgroup = one sample x 16 classes, 4 waves; a LANE owns a window step t, a WAVE owns the classes
// wave, wave + 4, wave + 8, wave + 12 of the group, and every lane walks k upwards with one predicated fmaf per class
// (`steps[k] == t`): each (b, c, t) is ONE fmaf chain in ascending k, whatever B, the grid or the neighbours are - no atomics, no
// cross-lane sum.  steps, pooled and the group's 16 rows of W are staged through LDS in tiles of 512 k and read as broadcasts,
// four k per instruction.  T > 64 takes one pass over k per 64 steps.  About C*T*K predicated FMAs per sample.
// A steps entry outside [0, T) equals no lane's t: it is compared, never used as an address.
#include "common.h"
#include "step_maps.h"

namespace {

constexpr int kTile = 512;      // k per LDS tile
constexpr int kGroup = 16;      // classes per workgroup
constexpr int kWaves = 4;
constexpr int kSlots = kGroup / kWaves;

__global__ __launch_bounds__(kWaves * 64) void step_maps_kernel(const float *__restrict__ pooled, const int32_t *__restrict__ steps,
                                                                const float *__restrict__ W, int K, int C, int T,
                                                                float *__restrict__ tam) {
  __shared__ __attribute__((aligned(16))) int32_t sst[kTile];
  __shared__ __attribute__((aligned(16))) float spl[kTile];
  __shared__ __attribute__((aligned(16))) float sw[kGroup][kTile];
  const int b = blockIdx.x, c0 = blockIdx.y * kGroup;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the wave's classes c0 + wave + 4 * i are ascending in i: the ones inside C are a prefix
  int nv = 0;
#pragma unroll
  for (int i = 0; i < kSlots; ++i) nv += (c0 + wave + kWaves * i < C) ? 1 : 0;
  const int32_t *st = steps + (long)b * K;
  const float *pl = pooled + (long)b * K;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int t = t0 + lane;
    float acc[kSlots];
#pragma unroll
    for (int i = 0; i < kSlots; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < K; k0 += kTile) {
      __syncthreads();      // the tile before this one has been read
      for (int i = threadIdx.x; i < kTile; i += kWaves * 64) {
        const bool in = k0 + i < K;
        sst[i] = in ? st[k0 + i] : -1;      // past K: a step no lane owns
        spl[i] = in ? pl[k0 + i] : 0.f;
      }
      for (int i = threadIdx.x; i < kGroup * kTile; i += kWaves * 64) {
        const int cl = i / kTile, kk = i - cl * kTile;
        sw[cl][kk] = (c0 + cl < C && k0 + kk < K) ? W[(long)(c0 + cl) * K + k0 + kk] : 0.f;
      }
      __syncthreads();
      const int kn = min(kTile, K - k0);
      for (int kk = 0; kk < kn; kk += 4) {      // (kTile % 4 == 0: the last four stay inside the tile, its padding matches no t)
        const int4 s4 = *(const int4 *)(sst + kk);
        const float4 p4 = *(const float4 *)(spl + kk);
#pragma unroll
        for (int i = 0; i < kSlots; ++i) {
          if (i < nv) {
            const float4 w4 = *(const float4 *)(&sw[wave + kWaves * i][kk]);
            acc[i] = s4.x == t ? fmaf(w4.x, p4.x, acc[i]) : acc[i];
            acc[i] = s4.y == t ? fmaf(w4.y, p4.y, acc[i]) : acc[i];
            acc[i] = s4.z == t ? fmaf(w4.z, p4.z, acc[i]) : acc[i];
            acc[i] = s4.w == t ? fmaf(w4.w, p4.w, acc[i]) : acc[i];
          }
        }
      }
    }
    if (t < T) {
#pragma unroll
      for (int i = 0; i < kSlots; ++i)
        if (i < nv) tam[((long)b * C + c0 + wave + kWaves * i) * T + t] = acc[i];
    }
  }
}

}  // namespace

int launch_step_maps(const float *pooled, const int32_t *steps, const float *W, int B, int K, int C, int T, float *tam,
                     hipStream_t s) {
  TN_REQUIRE(pooled && steps && W && tam, "step_maps: null argument");
  TN_REQUIRE(B > 0 && K > 0 && C > 0 && T > 0, "step_maps: bad shape");
  TN_REQUIRE((C + kGroup - 1) / kGroup <= 65535, "step_maps: too many classes");
  hipLaunchKernelGGL(step_maps_kernel, dim3(B, (C + kGroup - 1) / kGroup), dim3(kWaves * 64), 0, s, pooled, steps, W, K, C, T, tam);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}
