// Launchers of the fp32x3 training GEMMs (gemm_fp32x3.hip): fp32 in, fp32 out, fp32 accumulators, the products on the bf16
// matrix pipe as three bf16 terms per operand value.  The two forms the backbone training step (finetune.hip) uses.
#pragma once
#include <hip/hip_runtime.h>

// NT form, the arguments of launch_linear_f32 / launch_linear_f32_bnrelu (linear.h):
//   Y (M, N; row stride ldy) (+)= f(X) W^T (+ bias),  X (M, K; ldx), W (N, K; ldw),
//   f the identity (asc == ash == nullptr) or fmaxf(fmaf(x, asc[k], ash[k]), 0.f).
// Any M, N, K >= 1, any strides >= the extents, operands aligned to 4 bytes only.
int launch_linear_fp32x3(const float *X, int ldx, const float *asc, const float *ash, const float *Wt, int ldw, const float *bias, float *Y,
                         int ldy, int M, int N, int K, int accumulate, hipStream_t s);
// TN form, the arguments of launch_gemm_tn_f32 / launch_gemm_tn_f32_bnrelu (train.h):
//   C (M, N; row stride ldc) = A^T g(B) over the K rows of A (K, lda) and B (K, ldb),
//   g the identity (bsc == bsh == nullptr) or fmaxf(fmaf(b, bsc[n], bsh[n]), 0.f).
// ws / ws_floats: split-K scratch with the policy of the f32 launcher (null or too small: fewer or no slices); the slices are added
// in slice order, so the same arguments - workspace size included - give the same bits.
int launch_gemm_tn_fp32x3(const float *A, int lda, const float *Bm, int ldb, const float *bsc, const float *bsh, float *Cm, int ldc, int M,
                          int N, int K, hipStream_t s, float *ws, long ws_floats);
