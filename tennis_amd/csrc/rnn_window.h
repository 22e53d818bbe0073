// Launchers of the windowed recurrent / pooling kernels (rnn_window.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// gi [rows][2*G*H]: the i2h projection of every row of the feature matrix (both directions); centre / lo / hi [B] device int32:
// the window of sample b reads row clamp(centre[b] + (t - T/2) * stride, lo[b], hi[b]), clamped once more to [0, rows-1];
// pooled [B][2*H] = max over the T steps of concat(fwd, bwd).  nb: samples per workgroup, 0 = rnn_window_default_nb(gates)
// (4 or 6 for a GRU / 4 or 8 for an LSTM; the result does not depend on it).
int rnn_window_default_nb(int gates);
int launch_rnn_window(int gates, const float *gi, int ldgi, int rows, const float *whT, const float *bh, const int32_t *centre,
                      const int32_t *lo, const int32_t *hi, float *pooled, int B, int T, int stride, int H, int nb,
                      hipStream_t s, int32_t *steps = nullptr);
// steps [B][2*H] int32 or null: the window position t in [0, T-1] whose state each unit's maximum was read from, the smallest such t
// (the first-maximum rule of launch_pool_max_arg); pooled and everything else are the bits of the call without it
// the table form: idx [B][T] device int32, step t of sample b reads row clamp(idx[b*T + t], 0, rows-1) (a negative entry is row 0);
// a table that spells out a (centre, lo, hi, stride) window gives the bits of launch_rnn_window
int launch_rnn_window_rows(int gates, const float *gi, int ldgi, int rows, const float *whT, const float *bh, const int32_t *idx,
                           float *pooled, int B, int T, int H, int nb, hipStream_t s, int32_t *steps = nullptr);
// x [rows][F] -> y [B][F]: max / mean (tn_pool_kind) over the same gathered rows of x itself
int launch_temporal_pool_windows(const float *x, int rows, int F, const int32_t *centre, const int32_t *lo, const int32_t *hi,
                                 int B, int T, int stride, int kind, float *y, hipStream_t s, int32_t *arg = nullptr);
// arg [B][F] int32 or null (TN_POOL_MAX only): the first window position that holds the maximum
// ... and over the rows clamp(idx[b*T + t], 0, rows-1) of a table, t ascending as above
int launch_temporal_pool_rows(const float *x, int rows, int F, const int32_t *idx, int B, int T, int kind, float *y,
                              hipStream_t s, int32_t *arg = nullptr);
