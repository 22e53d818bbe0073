// Launcher of the temporal activation maps (step_maps.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// pooled [B][K] fp32, steps [B][K] int32, W [C][K] fp32 -> tam [B][C][T] fp32:
//   tam[b][c][t] = sum over the k with steps[b][k] == t, k ascending, of W[c][k] * pooled[b][k]      (one fmaf chain per (b, c, t))
// Every (b, c, t) is written; a step no unit names gets 0.0f; an entry of steps outside [0, T) is compared, never used as an index,
// and contributes nothing.  No atomics: the bits of sample b do not depend on B or on the grid.  K, C, T >= 1, C <= 65535 * 16.
int launch_step_maps(const float *pooled, const int32_t *steps, const float *W, int B, int K, int C, int T, float *tam,
                     hipStream_t s);
