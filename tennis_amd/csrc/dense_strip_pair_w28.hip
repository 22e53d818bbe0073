// dense_strip kernels of the 28 x 28 maps in the PAIRED form: two frames per workgroup, each wave walks half a frame (14 output
// rows where a quarter has 7; dense_strip_impl.h::DSGeomPair).  The same layer body (dense_strip_body.h) with the same LDS map,
// slot schedules and window registers as dense_strip_kernel<28, KS>: per output the same arithmetic in the same order, so the
// results are bit-identical to the one-frame launches.  What changes is how many rows share a wave's fixed work - the weight
// prologue (resident once, serving both frames), the cold first activation row, the window warm-up and the exposed last
// epilogue - and the seam: 15 or 16 bottleneck rows per 14 output rows where two quarters compute 17 or 18.  Half as many
// workgroups per launch: for calls that share the chip with a neighbouring stream's launch only (encoder_plan.h).
#include "dense_strip_impl.h"

namespace {

// the per-layer launch (K = 320 on the timed path; the others so that every link of the chain below can be run alone)
template <int KS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void dense_strip_pair_kernel(DenseStripArgs a) {
  constexpr int W = 28;
#define TN_STRIP_TID threadIdx.x
#define TN_STRIP_GEOM DSGeomPair<KS>
#include "dense_strip_body.h"
#undef TN_STRIP_GEOM
#undef TN_STRIP_TID
}

template <int KS>
__device__ __forceinline__ void dense_strip_pair_layer(const DenseStripArgs &a, const int tid_in) {
  constexpr int W = 28;
#define TN_STRIP_TID tid_in
#define TN_STRIP_GEOM DSGeomPair<KS>
#include "dense_strip_body.h"
#undef TN_STRIP_GEOM
#undef TN_STRIP_TID
}

// The block's first six strip layers (K = 128 ... 288, DSChain<28>) on the workgroup's two frames in one launch.  The boundary
// between two layers is dense_strip_kernel_chain's and its reasoning holds unchanged: layer l + 1 of a frame reads what the waves
// of THIS workgroup stored (both frames live on this CU; a wave reads its own frame only, across the seam the other half's
// rows), and the wait plus barrier covers all four waves.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void dense_strip_pair_kernel_chain(DenseStripChainArgs c) {
  using C = DSChain<28>;
  static_for<C::NL>([&](auto l_tag) TN_INL {
    constexpr int L = decltype(l_tag)::value;
    const DenseStripLayerDev d = c.layers[L];
    const DenseStripArgs a{c.buf, c.ldc, (C::KS0 + L) * 32, d.s1, d.t1, d.w1s, d.w3s, c.B, 28, 28, nullptr};
    int tid = threadIdx.x;      // (every layer derives its own lane geometry: dense_strip_kernel_chain)
    asm volatile("" : "+v"(tid));
    __builtin_assume(tid >= 0 && tid < 256);
    dense_strip_pair_layer<C::KS0 + L>(a, tid);
    if constexpr (L + 1 < C::NL) strip_layer_boundary();
  });
}

template <int KS>
int launch_strip_pair(const DenseStripArgs &a, hipStream_t s) {
  using G = DSGeomPair<KS>;
  TN_SET_ATTR_ONCE_PER_DEVICE(TN_HIP_CHECK(hipFuncSetAttribute((const void *)dense_strip_pair_kernel<KS>, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS_BYTES)));
  hipLaunchKernelGGL((dense_strip_pair_kernel<KS>), dim3(a.B / 2), dim3(256), G::LDS_BYTES, s, a);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}

}  // namespace

int launch_dense_strip_pair_w28(const DenseStripArgs &a, hipStream_t s) {
  TN_REQUIRE(a.B > 0 && a.B % 2 == 0, "dense_strip_pair: odd batch (a workgroup takes two frames)");
  switch (a.K / 32) {
    case 4: return launch_strip_pair<4>(a, s);
    case 5: return launch_strip_pair<5>(a, s);
    case 6: return launch_strip_pair<6>(a, s);
    case 7: return launch_strip_pair<7>(a, s);
    case 8: return launch_strip_pair<8>(a, s);
    case 9: return launch_strip_pair<9>(a, s);
    case 10: return launch_strip_pair<10>(a, s);
  }
  TN_REQUIRE(false, "dense_strip_pair: K out of range");
}

int launch_dense_strip_pair_chain_w28(const DenseStripChainArgs &c, hipStream_t s) {
  using C = DSChain<28>;
  TN_REQUIRE(c.B > 0 && c.B % 2 == 0, "dense_strip_pair_chain: odd batch (a workgroup takes two frames)");
  TN_REQUIRE(c.K0 == C::KS0 * 32 && c.nl == C::NL, "dense_strip_pair_chain: not the layer sequence the kernel was built for");
  TN_SET_ATTR_ONCE_PER_DEVICE(TN_HIP_CHECK(hipFuncSetAttribute((const void *)dense_strip_pair_kernel_chain, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES)));
  hipLaunchKernelGGL(dense_strip_pair_kernel_chain, dim3(c.B / 2), dim3(256), C::LDS_BYTES, s, c);
  TN_HIP_CHECK(hipGetLastError());
  return TN_OK;
}
