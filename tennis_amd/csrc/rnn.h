// Launchers of the recurrent / pooling / metric kernels (rnn.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// Dynamic LDS of a workgroup of nb batch rows: forward h | gates | c; BPTT dh (| dc) | pre-activation gradients | partial sums
inline size_t rnn_lds_fwd(int gates, int nb, int H) { return (size_t)(nb * H * 2 + nb * gates * H) * sizeof(float); }
inline size_t rnn_lds_bwd(int gates, int nb, int H) { return (size_t)(nb * H * (gates == 4 ? 2 : 1) + 2 * nb * gates * H) * sizeof(float); }
// The big route's split of a W_hh column: kr values in registers, kl in LDS (as much as the 160 KB hold), the rest streamed; threads
// is the block-size bound its kernels are compiled for.  Forward and BPTT instantiate their kernels from this one function.
struct tn_rnn_big_split { int kr, kl, threads; };
constexpr tn_rnn_big_split rnn_big_split(int gates) {
  return gates == 3 ? tn_rnn_big_split{112, 48, 768} : tn_rnn_big_split{64, 32, 1024};
}
// Which instantiation the forward kernel (rnn.hip, with or without `save`) and the BPTT kernel (rnn_bptt.hip) run for a shape - the
// one policy of both, so that the kernel that writes `save` and the one that reads it agree on the rows per workgroup:
//   nb   rows per workgroup: 4 when that still gives every CU a workgroup, else 1 (latency-bound small batches)
//   kr   register-resident prefix of each W_hh column (128 / 96 / 64 / 0), bounded by the VGPR budget the block size leaves; 0 with
//        four rows per workgroup (the unrolled prefix would spill); not read on the big route, whose split is rnn_big_split
//   big  one row per workgroup and a column that does not fit the registers (H = 256): registers + LDS + stream, h through DPP
//   lds_fwd / lds_bwd  dynamic LDS of the forward / the BPTT kernel, on the big route with the LDS share of the weights
struct tn_rnn_route { int nb, kr, big; size_t lds_fwd, lds_bwd; };
inline tn_rnn_route rnn_route(int gates, int B, int H, int dirs) {
  const int threads = gates * H;
  tn_rnn_route r;
  r.nb = ((B + 3) / 4) * dirs >= 256 ? 4 : 1;
  r.kr = r.nb == 4 ? 0 : (threads <= 512 && H >= 128) ? 128 : (threads <= 768 && H >= 96) ? 96 : H >= 64 ? 64 : 0;
  r.big = r.nb == 1 && H == 256;
  const size_t wl = r.big ? (size_t)rnn_big_split(gates).kl * threads * sizeof(float) : 0;
  r.lds_fwd = rnn_lds_fwd(gates, r.nb, H) + wl;
  r.lds_bwd = rnn_lds_bwd(gates, r.nb, H) + wl;
  return r;
}
// The wide recurrence, 1024 < gates*H <= 2048 (LSTM up to H = 512, GRU up to H = 680): a workgroup cannot give every gate row a thread
// of its own, so a thread owns `rows` = 2 of them, j and j + threads (the second one guarded against gates*H).  Like rnn_route the one
// policy of the forward kernel (rnn.hip) and of the BPTT kernel (rnn_bptt.hip), so that both agree on the rows per workgroup:
//   threads  the block: half the gate rows, rounded up to whole waves (<= 1024)
//   rows     gate rows per thread (2)
//   nb       batch rows per workgroup, rnn_route's threshold: 4 when that still gives every CU a workgroup, else 1
//   lds_fwd  dynamic LDS of the forward kernel
//   lds_bwd  ... of the BPTT kernel; above 64 KiB at nb = 4 from H = 412 (LSTM) / 588 (GRU): the launcher raises the kernel's limit
// The arithmetic also holds for gates*H <= 1024, which only the test hook tn_dbg_rnn_force_wide sends this way.
struct tn_rnn_wide_route { int threads, rows, nb; size_t lds_fwd, lds_bwd; };
inline tn_rnn_wide_route rnn_wide_route(int gates, int B, int H, int dirs) {
  const int GH = gates * H;
  tn_rnn_wide_route r;
  r.rows = 2;
  r.threads = ((GH + 1) / 2 + 63) / 64 * 64;
  r.nb = ((B + 3) / 4) * dirs >= 256 ? 4 : 1;
  r.lds_fwd = rnn_lds_fwd(gates, r.nb, H);
  r.lds_bwd = rnn_lds_bwd(gates, r.nb, H);
  return r;
}
// true for the shapes the wide kernels serve: every gates*H > 1024, and every shape while tn_dbg_rnn_force_wide is on
bool rnn_takes_wide(int gates, int H);
void rnn_set_force_wide(bool on);
// launches of the wide kernels so far, forward and BPTT (what tn_dbg_rnn_wide_launches reports: a test can tell which family ran)
void rnn_count_wide_launch();
long rnn_wide_launches();
int launch_rnn_recurrent(int gates, const float *gi, int ldgi, const float *whT, const float *bh,
                         const int32_t *valid_len, float *seq, int ldo, float *h_last, float *c_last, int B, int T,
                         int H, int dirs, hipStream_t s, float *save = nullptr);
// save (training, rnn_bptt.hip's BPTT): per (dir, row) the gate activations of every step, [dirs][B*T][(G+1)*H] =
// GRU r | z | n | (W_hn h + b_hn), LSTM i | f | g | o | c_t
int launch_temporal_pool(const float *x, int B, int T, int F, int kind, float *y, hipStream_t s);
int launch_prf1(const float *logits, const int32_t *labels, int rows, int classes, int64_t *mat, hipStream_t s);
