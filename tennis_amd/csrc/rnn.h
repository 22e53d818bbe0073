// Launchers of the recurrent / pooling / metric kernels (rnn.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// Which instantiation the forward kernel (rnn.hip, with or without `save`) and the BPTT kernels (train.hip) run for a shape - the
// one policy of both, so that the kernel that writes `save` and the one that reads it agree on the rows per workgroup:
//   nb   rows per workgroup: 4 when that still gives every CU a workgroup, else 1 (latency-bound small batches)
//   kr   register-resident prefix of each W_hh column (128 / 96 / 64 / 0), bounded by the VGPR budget the block size leaves; 0 with
//        four rows per workgroup (the unrolled prefix would spill); not read on the big route, whose kernels carry their own split
//   big  one row per workgroup and a column that does not fit the registers (H = 256): registers + LDS + stream, h through DPP
struct tn_rnn_route { int nb, kr, big; };
inline tn_rnn_route rnn_route(int gates, int B, int H, int dirs) {
  const int threads = gates * H;
  tn_rnn_route r;
  r.nb = ((B + 3) / 4) * dirs >= 256 ? 4 : 1;
  r.kr = r.nb == 4 ? 0 : (threads <= 512 && H >= 128) ? 128 : (threads <= 768 && H >= 96) ? 96 : H >= 64 ? 64 : 0;
  r.big = r.nb == 1 && H == 256;
  return r;
}
int launch_rnn_recurrent(int gates, const float *gi, int ldgi, const float *whT, const float *bh,
                         const int32_t *valid_len, float *seq, int ldo, float *h_last, float *c_last, int B, int T,
                         int H, int dirs, hipStream_t s, float *save = nullptr);
// save (training, train.hip's BPTT): per (dir, row) the gate activations of every step, [dirs][B*T][(G+1)*H] =
// GRU r | z | n | (W_hn h + b_hn), LSTM i | f | g | o | c_t
int launch_temporal_pool(const float *x, int B, int T, int F, int kind, float *y, hipStream_t s);
int launch_prf1(const float *logits, const int32_t *labels, int rows, int classes, int64_t *mat, hipStream_t s);
