/* libtennis_hip.so - instrumentation and test hooks (NOT part of the drop-in surface of include/tennis_hip.h).
 *
 * A maintainer binding the reference's path needs tennis_hip.h only.  What is declared here is exported by the same library for
 * this repo's own tests/ (single kernels pinned against the oracle at ragged sizes), bench.py (per-kernel HIP-event timing for
 * the roofline object) and scripts/ (tuning): no reference call site stands behind any of it. */
#ifndef TENNIS_HIP_DEBUG_H
#define TENNIS_HIP_DEBUG_H
#include "tennis_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Per-kernel-family timing returned by tn_densenet121_profile. */
typedef struct {
  char name[32];      /* kernel family, e.g. "conv3x3_bnrelu" */
  int launches;       /* launches of this family in one forward */
  double ms;          /* summed HIP-event time of those launches */
  double flops;       /* algorithmic FLOPs of those launches (2*MACs of the convs) */
  double bytes;       /* algorithmic bytes moved (activations+weights, once each) */
} tn_kernel_stat;


/* Same forward, but every launch is bracketed by HIP events on the ctx stream;
 * fills up to max_stats families and syncs.  For bench.py's roofline. */
int tn_densenet121_profile(tn_encoder *enc, const void *x, tn_layout layout, int batch, float *feat,
                           tn_kernel_stat *stats, int max_stats, int *n_stats);

/* tn_densenet121_forward_class_maps under the same event timer (one stream): the family "class_maps" stands beside
 * "head_bnrelu_avgpool7", which reads the same map once. */
int tn_dbg_profile_class_maps(tn_encoder *enc, const void *x, tn_layout layout, int batch, float *feat, const tn_dense *classes,
                              float *maps, tn_kernel_stat *stats, int max_stats, int *n_stats);
/* class_maps_kernel (csrc/class_maps.hip) alone on a caller's DEVICE map (B,H,W,C) NHWC: fp16 x_f16, or - x32 non-NULL - fp32 (x_f16
 * is then not read).  scale / shift (C) and wd (classes, C PH PW) device fp32, maps (B, classes, 7 PH, 7 PW) device fp32.  Any
 * B, H >= 7 PH, W >= 7 PW, C % 8 == 0, classes in [1, 64]; everything else is refused.  n_seq / depth (either may be NULL): the longest
 * sequential fp32 accumulation of a lane at this C and the levels of the cross-lane reduction, the two constants of the error
 * bound (n_seq + depth + 4) 2^-24 S.  Synchronous. */
int tn_dbg_class_maps(tn_ctx *ctx, const void *x_f16, const float *x32, int B, int H, int W, int C, const float *scale, const float *shift,
                      const float *wd, int PH, int PW, int classes, float *maps, int *n_seq, int *depth);

/* Test hook: copy an internal NHWC fp16 activation of the LAST forward to a host
 * fp32 buffer.  tap in {"stem","pool0","stage1".."stage4","trans1".."trans3",
 * "stage<k>_l0_bottleneck"}; returns the element count through *numel. */
int tn_densenet121_read_tap(tn_encoder *enc, const char *tap, int batch, float *out_host,
                            size_t capacity, size_t *numel);

int tn_jpeg_sync_passes(const tn_jpeg *j);   /* diagnostic: decoder passes the last call needed to synchronise */

/* ---- test hooks (used by tests/ only) -------------------------------------- */
/* Run ONE encoder kernel on caller-provided device activations (fp16 NHWC) with
 * host fp32 weights in Gluon layout, folded/packed exactly as
 * tn_densenet121_create does; synchronous.  They let the parity tests pin each
 * kernel against the oracle at ragged sizes and channel offsets. */
int tn_dbg_conv1x1(tn_ctx *ctx, const void *x_f16, int ldx, int K, const float *scale_host,
                   const float *shift_host, const float *w_host, int N, void *y_f16, int ldy, int yoff,
                   int M, int pool, int H, int W);
int tn_dbg_conv3x3(tn_ctx *ctx, const void *x_f16, const float *scale_host, const float *shift_host,
                   const float *w_host, void *y_f16, int ldy, int yoff, int B, int H, int W);
/* Tuning hooks: asynchronous single launches on device-resident, pre-converted
 * operands (fp16 [N][K] 1x1 weights; tn_dbg_pack_conv3x3 image for the 3x3:
 * 2 x 72*64*8 halves, the 32x32x16 and the 16x16x32 MFMA operand layouts). */
int tn_dbg_pack_conv3x3(const float *w_host, uint16_t *out_host);
int tn_dbg_conv1x1_dev(tn_ctx *ctx, const void *x_f16, int ldx, int K, const float *scale, const float *shift,
                       const void *w_f16, int N, void *y_f16, int ldy, int yoff, int M, int pool, int H, int W,
                       int variant);
/* variant: the low 16 bits the kernel choice (9: weights fetched inside the loop); bit 17: exact weights, wp_f16 = the hi image
 * followed by the lo image (two tn_dbg_pack_conv3x3 images). */
int tn_dbg_conv3x3_dev(tn_ctx *ctx, const void *x_f16, const float *scale, const float *shift,
                       const void *wp_f16, void *y_f16, int ldy, int yoff, int B, int H, int W, int variant);
/* tn_dbg_conv1x1_dev with the remaining arguments of the launcher (csrc/conv1x1.hip, csrc/trans_ws.hip): bias (device fp32 [N],
 * added before the rounding; or NULL), clamp (scale / shift hold lo / hi and the operand is clamp(x, lo, hi)), y32 (device fp32
 * [M][ld32], the un-rounded result once more; or NULL) and wfrag (device: the caller's MFMA-order image of w, which sends a
 * supported transition to the warp-specialised kernel; or NULL).  variant bit 17: w is [N][2 Kp] = [hi | lo].  Asynchronous.
 * Refuses y32 with ld32 < N and wfrag with a geometry the warp-specialised kernel does not support. */
int tn_dbg_conv1x1_ex(tn_ctx *ctx, const void *x_f16, int ldx, int K, const float *scale, const float *shift, const void *w_f16, int N,
                      void *y_f16, int ldy, int yoff, int M, int pool, int H, int W, int variant, const float *bias, int clamp,
                      float *y32, int ld32, const void *wfrag);
/* The warp-specialised transition with the head folded into its epilogue (csrc/trans_ws.hip): tn_dbg_conv1x1_ex's pooling form with
 * wfrag, plus feat (device fp32, row pitch ldfeat >= N) and head_s / head_t (device fp32 [N], 16-byte aligned).  Frame f's row of feat
 * receives in columns [0, N) the mean over the frame's 49 pooled pixels of relu(head_s[n] * result + head_t[n]), the un-rounded
 * results summed in pixel order as the head kernel sums them; y32 is not written.  Refused before any launch: N other than 512, a
 * map other than 14 x 14 (the frame has to be one tile).  Asynchronous. */
int tn_dbg_conv1x1_head(tn_ctx *ctx, const void *x_f16, int ldx, int K, const float *scale, const float *shift, const void *w_f16, int N,
                        void *y_f16, int ldy, int yoff, int M, int pool, int H, int W, float *y32, int ld32, const void *wfrag,
                        float *feat, const float *head_s, const float *head_t, int ldfeat);
/* w [N][K] fp16 -> the fragment image the warp-specialised transition reads, [K / 16][N / 32][64 lanes][8] (lane l: row l & 31,
 * k offset 8 (l >> 5)): the host function tn_densenet121_create packs with (touches no device), and the device kernel. */
int tn_dbg_pack_trans_frags(const uint16_t *w_f16_host, int N, int K, uint16_t *out_host);
int tn_dbg_pack_trans_frags_dev(tn_ctx *ctx, const void *w_f16, int N, int K, void *out_f16);
int tn_dbg_dense_layer_dev(tn_ctx *ctx, void *buf_f16, int ldc, int K, const float *s1, const float *t1,
                           const void *w1_f16, const float *s2, const float *t2, const void *w3p_f16, int B,
                           int H, int W, unsigned long long *ts /* NULL or stamps */, int variant /* 0 auto, 1 big, 2 small */);
/* nchain consecutive fused dense layers (K0, K0 + 32, ...) as one chained launch of the tile kernel (16x16, 14x14, 7x7): s1 ... w3p_f16
 * are host arrays of nchain device pointers, one per layer, in the forms tn_dbg_dense_layer_dev takes; variant likewise (bit 17:
 * exact weights; bit 19: nchain is passed on without the layer array, which the launcher has to refuse).  Synchronous. */
int tn_dbg_dense_chain_dev(tn_ctx *ctx, void *buf_f16, int ldc, int K0, int nchain, const float *const *s1, const float *const *t1,
                           const void *const *w1_f16, const float *const *s2, const float *const *t2, const void *const *w3p_f16,
                           int B, int H, int W, int variant);
int tn_dbg_linear(tn_ctx *ctx, const float *x, const float *w, const float *bias, float *y, int M, int N,
                  int K);
/* The reduction behind tn_densenet121_input_means on its own: out[c] (device fp32, K values) = mean over `rows` rows of the device
 * fp16 matrix x (rows, ld) of relu(scale[c] x + shift[c]), or with `clamp` of clamp(x, lo = scale[c], hi = shift[c]); scale / shift
 * device fp32, scratch a device buffer of scratch_bytes >= 32 K doubles.  Synchronous. */
int tn_dbg_channel_mean(tn_ctx *ctx, const void *x_f16, int ld, int K, const float *scale, const float *shift, int64_t rows,
                        void *scratch, size_t scratch_bytes, float *out, int clamp);
/* The first kernels of a forward on their own: the pooled stem map (conv 7x7/2 + BatchNorm + ReLU + MaxPool 3x3/2) of B frames x
 * (device, in `layout`) into y (device fp16, (B, Hp, Wp) pixels of 64 channels at row stride ldy).  conv0's weights (64,3,7,7) and
 * batchnorm0's parameters are host fp32 and folded as tn_densenet121_create folds them; centre_host: the 64 channel means m_c the
 * stored map is centred by, or NULL; exact: hi + lo weights (TN_ENC_EXACT_WEIGHTS); fused: the fused kernel, otherwise the stem
 * kernel into a map of the hook's own followed by the max pool kernel (TN_NO_FUSE).  Synchronous. */
int tn_dbg_stem(tn_ctx *ctx, const float *w0_host, const float *gamma_host, const float *beta_host, const float *mean_host,
                const float *var_host, const float *centre_host, int exact, int fused, int layout, int B, int H, int W,
                const void *x, void *y_f16, int ldy);
/* MaxPool2D(3, 2, pad 1) of a device fp16 NHWC map (B,H,W,C) into y (B, Ho, Wo) at row stride ldy >= C.  Synchronous. */
int tn_dbg_maxpool(tn_ctx *ctx, const void *x_f16, int B, int H, int W, int C, void *y_f16, int ldy, int Ho, int Wo);
/* The last kernel: BatchNorm + ReLU + AvgPool2D(7) + NCHW flatten of a device NHWC map (B,H,W,C) into feat (B, C PH PW) device fp32,
 * read from the fp16 map x_f16 or - x32 non-NULL - from the fp32 map x32 (x_f16 is then ignored); scale / shift device fp32.
 * Synchronous. */
int tn_dbg_head(tn_ctx *ctx, const void *x_f16, const float *x32, int B, int H, int W, int C, const float *scale, const float *shift,
                float *feat, int PH, int PW);
/* The strip-streaming fused dense layer (csrc/dense_strip.hip; 56x56 / 28x28 blocks, K <= 320): fp32 (128,K) 1x1 weights
 * with the folded scale / shift (128 each) of the BatchNorm behind them, and (32,128,3,3) 3x3 weights -> the MFMA
 * A-fragment images the kernel keeps resident in LDS ((K+16)*128 and 36864 halves; either output may be NULL), and one
 * asynchronous launch on device-resident packed operands. */
int tn_dbg_pack_strip(const float *w1_host, int K, const float *s2_host, const float *t2_host, uint16_t *w1s_out,
                      const float *w3_host, uint16_t *w3s_out);
int tn_dbg_dense_strip_dev(tn_ctx *ctx, void *buf_f16, int ldc, int K, const float *s1, const float *t1,
                           const void *w1s_f16, const void *w3s_f16, int B, int H, int W,
                           unsigned long long *ts /* NULL or 128 s_memtime stamps per frame */);
/* The same layer in the paired launch geometry of the 28x28 maps (csrc/dense_strip_pair_w28.hip): two frames per workgroup, each
 * wave walks half a frame; bit-identical to tn_dbg_dense_strip_dev on the same input.  28x28 and K = 128 ... 320 only; an odd B is
 * refused without a launch.  ts: NULL or 128 stamps per workgroup (B / 2 of them).  The chained form runs nl = 6 layers from
 * K0 = 128 in one launch, as six calls of tn_dbg_dense_strip_dev in order would; its operand arrays hold one device pointer per
 * layer, and it is synchronous. */
int tn_dbg_dense_strip_pair_dev(tn_ctx *ctx, void *buf_f16, int ldc, int K, const float *s1, const float *t1,
                                const void *w1s_f16, const void *w3s_f16, int B, int H, int W, unsigned long long *ts);
int tn_dbg_dense_strip_pair_chain_dev(tn_ctx *ctx, void *buf_f16, int ldc, int K0, int nl, const float *const *s1,
                                      const float *const *t1, const void *const *w1s_f16, const void *const *w3s_f16, int B, int H,
                                      int W);
/* *count: how many launches of the process took the paired 28x28 strip kernels so far.  The instrumented pass never takes that
 * route (it does not share the chip with a neighbouring call), so this count is how a test sees it. */
int tn_dbg_strip_pair_launches(int64_t *count);
/* *count: how many launches of the process ran with the head folded in so far (the last transition and the 7x7 block kernel: two
 * per frame range of a forward on that route).  A profile cannot show the route; this count does. */
int tn_dbg_head_fused_launches(int64_t *count);
/* *fused: 1 where a forward of that input size, create flags (and TN_* environment), batch and pass folds the head into the last
 * transition and the 7x7 block kernel (csrc/encoder_plan.h::enc_head_fused), 0 where it keeps the fp32 side copy and the head launch.
 * class_maps: the call is tn_densenet121_forward_class_maps.  Touches no device. */
int tn_dbg_head_fused(int height, int width, int flags, int batch, int calibrate, int class_maps, int *fused);

/* The event decoder's geometry (csrc/event_runs.hip): *tile = positions per workgroup of its score and scatter kernels, *scan_block =
 * tile counts its one scan workgroup takes per step (more tiles than that make it loop).  Tests place their edge shapes from these.
 * Touches no device. */
int tn_dbg_event_decoder_geometry(int *tile, int *scan_block);

/* The switch-cost path decoder's geometry: *tile = positions of a video its forward and backtrack kernels take per step (the rows
 * staged into LDS while the walking wave consumes the tile before).  Touches no device. */
int tn_dbg_event_decoder_switch_geometry(int *tile);

/* The transition-matrix path decoder's geometry: *tile = positions of a video its forward and backtrack kernels take per step,
 * *pitch16 / *pitch64 = bytes of a position's row of back-pointers in a handle of max_classes <= 16 / above.  Touches no device. */
int tn_dbg_event_decoder_transition_geometry(int *tile, int *pitch16, int *pitch64);

/* Device bytes the handle holds: what tn_event_decoder_create allocated, plus the path workspace once the first
 * tn_event_decoder_run_switch has allocated it, plus the back-pointer workspace once the first tn_event_decoder_run_transitions has,
 * plus the posterior workspace (2 * max_positions * pitch * 4 bytes) once the first tn_event_decoder_run_posteriors has.
 * Touches no device. */
int tn_dbg_event_decoder_workspace_bytes(const tn_event_decoder *d, size_t *bytes);

/* The LDS-resident 7x7 dense block (csrc/dense_block7.hip): nl layers from K0 input channels in ONE launch on a device
 * concat buffer (B,7,7,ldc) fp16.  w1_all: the (128, K_l) 1x1 weights one after the other (K_l = K0 + 32 l); s1_all / t1_all
 * folded BN1 scale / shift (K_l each); s2_all / t2_all folded BN2 scale / shift (128 per layer); w3_all nl x (32,128,3,3). */
int tn_dbg_block7_create(tn_ctx *ctx, int K0, int nl, const float *w1_all, const float *s1_all, const float *t1_all,
                         const float *s2_all, const float *t2_all, const float *w3_all, void **out);
int tn_dbg_block7_run(void *handle, void *buf_f16, int ldc, int B);
int tn_dbg_block7_run_ts(void *handle, void *buf_f16, int ldc, int B,
                         unsigned long long *ts /* NULL or 128 per frame: s_memtime stamps of wave 0 (start, then 5 per layer) */);
/* ... with the un-rounded fp32 side copy of the appended channels (side: device fp32 (B,7,7,ldc), or NULL), or with the head folded
 * into the append (feat: device fp32, row pitch ldfeat >= K0 + 32 nl; head_s / head_t: device fp32 indexed by the concat buffer's
 * channel, 16-byte aligned): frame f's row of feat receives in columns [K0, K0 + 32 nl) the mean over the 49 pixels of
 * relu(head_s[c] * result + head_t[c]); side is then not written. */
int tn_dbg_block7_run_head(void *handle, void *buf_f16, int ldc, int B, float *side, float *feat, const float *head_s, const float *head_t,
                           int ldfeat, unsigned long long *ts);
void tn_dbg_block7_destroy(void *handle);

/* The streamed 14x14 dense block (csrc/dense_block14.hip; reference call site models/vision/definitions.py:30, the third dense
 * block of gluoncv's DenseNet-121): nl layers from K0 >= 256 input channels in ONE launch on a device concat buffer (B,14,14,ldc)
 * fp16; operands as tn_dbg_block7_create.  The handle owns the packed weight stream and the kernel's working copy of the frames. */
int tn_dbg_block14_create(tn_ctx *ctx, int K0, int nl, const float *w1_all, const float *s1_all, const float *t1_all,
                          const float *s2_all, const float *t2_all, const float *w3_all, void **out);
int tn_dbg_block14_run(void *handle, void *buf_f16, int ldc, int B);
int tn_dbg_block14_run_ts(void *handle, void *buf_f16, int ldc, int B,
                          unsigned long long *ts /* NULL or 64 per frame (160 in a -DTN_B14_STAMPS build): s_memtime stamps of wave 0, one per layer */);
void tn_dbg_block14_destroy(void *handle);
/* the streamed 28x28 dense block (csrc/dense_block28.hip), same operand convention */
int tn_dbg_block28_create(tn_ctx *ctx, int K0, int nl, const float *w1_all, const float *s1_all, const float *t1_all,
                          const float *s2_all, const float *t2_all, const float *w3_all, void **out);
int tn_dbg_block28_run(void *handle, void *buf_f16, int ldc, int B);
int tn_dbg_block28_run_ts(void *handle, void *buf_f16, int ldc, int B, unsigned long long *ts);
void tn_dbg_block28_destroy(void *handle);

/* The training kernels of the fine-tuning step (csrc/train.hip, linear.hip, finetune.hip) through the launchers the step calls; all
 * operands device fp32, synchronous.
 * tn_dbg_gemm_tn: C (M, N; row stride ldc) = A^T B over K rows, A (K, lda), B (K, ldb); bsc / bsh non-NULL: B -> relu(B bsc[n] + bsh[n])
 * first.  workspace / workspace_floats: the caller's split-K scratch (NULL: never split) - it decides whether and how far K is split. */
int tn_dbg_gemm_tn(tn_ctx *ctx, const float *A, int lda, const float *B, int ldb, const float *bsc, const float *bsh, float *Cm, int ldc,
                   int M, int N, int K, float *workspace, int64_t workspace_floats);
/* Y (M, N; row stride ldy) (+)= relu(X asc[k] + ash[k]) W^T (+ bias), X (M, ldx), W (N, ldw); accumulate: add to Y. */
int tn_dbg_linear_bnrelu(tn_ctx *ctx, const float *X, int ldx, const float *asc, const float *ash, const float *W, int ldw,
                         const float *bias, float *Y, int ldy, int M, int N, int K, int accumulate);
/* The same two products through the fp32x3 launchers (csrc/gemm_fp32x3.hip), what the step runs in TN_MATMUL_FP32X3: the arguments
 * of tn_dbg_linear_bnrelu (asc / ash NULL together: no operand transform) and of tn_dbg_gemm_tn. */
int tn_dbg_linear_fp32x3(tn_ctx *ctx, const float *X, int ldx, const float *asc, const float *ash, const float *W, int ldw,
                         const float *bias, float *Y, int ldy, int M, int N, int K, int accumulate);
int tn_dbg_gemm_tn_fp32x3(tn_ctx *ctx, const float *A, int lda, const float *B, int ldb, const float *bsc, const float *bsh, float *Cm,
                          int ldc, int M, int N, int K, float *workspace, int64_t workspace_floats);
/* Training-mode BatchNorm + ReLU of an (M, C) matrix x of row stride ld >= C: mean / var (C each, biased), y (M, C contiguous).
 * dy (M, C contiguous) non-NULL: also dgamma, dbeta (C each) and dx (row stride ldd), assigned or accumulated. */
/* C (M, N; row stride ldc) = A (M, K; row stride lda) B (K, N; row stride ldb), both row-major: the input gradient of the
 * CNN-RNN step's bi-RNN head, dX = dGI W_ih (csrc/gemm_nn.hip). */
int tn_dbg_gemm_nn(tn_ctx *ctx, const float *A, int lda, const float *B, int ldb, float *Cm, int ldc, int M, int N, int K);
int tn_dbg_bn_train(tn_ctx *ctx, const float *x, int ld, int64_t M, int C, const float *gamma, const float *beta, float *mean, float *var,
                    float *y, const float *dy, float *dgamma, float *dbeta, float *dx, int ldd, int accumulate);
/* The training steps' operator kernels, each alone (csrc/finetune.hip, csrc/train.hip), through the launchers the steps call, on the
 * context's stream, synchronous; all operands device fp32 (labels, valid_len, arg: device int32), NHWC.  Each hook refuses with
 * TN_ERR_INVALID and a message, before anything is launched: null pointers, counts <= 0, a row stride below its column count, and
 * what is listed with it.  docs/numerics.md, "The training steps' operator kernels, alone", has the bars they are held to.
 *   ft_im2col7: x (B, H, W, 3) -> col (B H/2 W/2, 147), 7x7 stride 2 pad 3, columns (ky, kx, c).  H, W even.
 *   ft_im2col3: a (B, H, W, C) -> col (B H W, 9 C), 3x3 pad 1, columns (ky, kx, c); sc / sh (C each, together or both NULL): the source
 *     goes through relu(a sc[c] + sh[c]), padding stays 0.  ft_col2im3: its adjoint, dcol -> da (B, H, W, C).  Both: C % 4 == 0 and
 *     every pointer 16-byte aligned.
 *   ft_maxpool: 3x3 stride 2 pad 1, a (B, H, W, C) -> y (B H/2 W/2 rows of stride ldy) when y is given; dy (rows of stride ldy) and da
 *     (B, H, W, C) given together: the gradient, to the first maximum of a window in (ky, kx) order.  H, W even.
 *   ft_avgpool2: 2x2 stride 2; z with y: the forward, dy with dz: the gradient; layouts of ft_maxpool.  H, W even.
 *   ft_gap: a (B, P, C) with f (B, C): the mean over P; df (B, C) with da (B, P, C): the gradient df / P.
 *   ft_bn_fold: sc = gamma / sqrt(var + 1e-5), sh = beta - mean sc.  ft_bn_running: running = 0.9 running + 0.1 batch, in place.
 *   pool_max_arg: x (B, T, F) -> y (B, F), arg (B, F) the first maximum over T; dpooled (B, F) with dseq (B, T, F): then the scatter of
 *     dpooled to step arg, zeros elsewhere.
 *   softmax_ce: loss (B) = -log softmax(logits (B, C))[label], dlogits = softmax - onehot.  labels_host: the host copy of labels; a
 *     label outside [0, C) is refused (the kernel indexes by it unchecked).
 *   dense_bwd: dwd (C, K) = dlogits^T pooled, dbd (C) = column sums of dlogits (B, C), dpooled (B, K) = dlogits wd.
 *   colsum: out (cols) = column sums of A (rows, lda).
 *   sgd_momentum: mom = momentum mom - lr (rescale g + wd w), w += mom.  adam: m, v, w of MXNet's Adam at the 1-based update count
 *     step, the bias correction folded into the rate.  scale: a device float that multiplies g first (the clipped instantiation), or
 *     NULL (the plain one).
 *   stage_frames: y (B, T, frame_floats) = x with zeros in the slots t >= valid_len[b].  frame_floats % 4 == 0, 16-byte aligned.
 *   transpose: dst (cols, rows) = src (rows, cols)^T. */
int tn_dbg_ft_im2col7(tn_ctx *ctx, const float *x, int B, int H, int W, float *col);
int tn_dbg_ft_im2col3(tn_ctx *ctx, const float *a, int B, int H, int W, int C, const float *sc, const float *sh, float *col);
int tn_dbg_ft_col2im3(tn_ctx *ctx, const float *dcol, int B, int H, int W, int C, float *da);
int tn_dbg_ft_maxpool(tn_ctx *ctx, const float *a, int B, int H, int W, int C, float *y, int ldy, const float *dy, float *da);
int tn_dbg_ft_avgpool2(tn_ctx *ctx, const float *z, int B, int H, int W, int C, float *y, int ldy, const float *dy, float *dz);
int tn_dbg_ft_gap(tn_ctx *ctx, const float *a, int B, int P, int C, float *f, const float *df, float *da);
int tn_dbg_ft_bn_fold(tn_ctx *ctx, const float *mean, const float *var, const float *gamma, const float *beta, int C, float *sc, float *sh);
int tn_dbg_ft_bn_running(tn_ctx *ctx, float *rmean, float *rvar, const float *mean, const float *var, int C);
int tn_dbg_pool_max_arg(tn_ctx *ctx, const float *x, int B, int T, int F, float *y, int32_t *arg, const float *dpooled, float *dseq);
int tn_dbg_softmax_ce(tn_ctx *ctx, const float *logits, const int32_t *labels, const int32_t *labels_host, int B, int C, float *loss,
                      float *dlogits);
int tn_dbg_dense_bwd(tn_ctx *ctx, const float *dlogits, const float *pooled, const float *wd, int B, int C, int K, float *dwd, float *dbd,
                     float *dpooled);
int tn_dbg_colsum(tn_ctx *ctx, const float *A, int lda, int rows, int cols, float *out);
int tn_dbg_sgd_momentum(tn_ctx *ctx, float *w, const float *g, float *mom, int64_t n, float lr, float momentum, float wd, float rescale,
                        const float *scale);
int tn_dbg_adam(tn_ctx *ctx, float *w, const float *g, float *m, float *v, int64_t n, float lr, float beta1, float beta2, float epsilon,
                int64_t step, const float *scale);
int tn_dbg_stage_frames(tn_ctx *ctx, const float *x, const int32_t *valid_len, int B, int T, int64_t frame_floats, float *y);
int tn_dbg_transpose(tn_ctx *ctx, const float *src, int rows, int cols, float *dst);
/* tn_gnmt_trainer_forward_backward that also leaves d loss / d src in dsrc (batch * steps, input_size; row stride ldd, DEVICE,
 * assigned): the gradient the frame-mode step (tn_gnmt_frames_trainer_*) hands to the backbone.  Rows at or past src_valid_len[b]
 * come out 0. */
int tn_dbg_gnmt_trainer_src_grad(tn_gnmt_trainer *t, const float *src, const int32_t *src_valid_len, const int32_t *tgt, int ld,
                                 const int32_t *tgt_valid_len, int batch, int steps, int tgt_len, float *loss, float *logits_out,
                                 float *dsrc, int ldd);
/* The gathered i2h product of tn_gnmt_trainer_forward_backward_rows / tn_gnmt_encode_rows skips the k-loop of a workgroup whose rows
 * are all padding.  on = 0 launches the instantiation compiled without that skip (same results), so that the skip can be measured
 * against it; on = 1 (the default) restores it.  Process-wide. */
int tn_dbg_rows_pad_skip(int on);

/* Which instantiation the recurrent kernels run for a shape (csrc/rnn.h rnn_route, the one policy of launch_rnn_recurrent and of the
 * BPTT launcher of csrc/rnn_bptt.hip): gates 3 GRU / 4 LSTM, B batch rows, H hidden, dirs 1 | 2.  *nb rows per workgroup (1 | 4), *kr the
 * register-resident prefix of a W_hh column (0 | 64 | 96 | 128; 0 at nb = 4; not read when *big), *big 1 for the registers + LDS +
 * stream form (H = 256 at nb = 1).  Host arithmetic only: touches no device. */
int tn_dbg_rnn_route(int gates, int B, int H, int dirs, int *nb, int *kr, int *big);

/* The dispatch policy of the wide recurrent kernels (csrc/rnn.h rnn_wide_route), which serve 1024 < gates*H <= 2048 with two gate rows
 * per thread: *threads the block (whole waves, <= 1024), *rows the gate rows per thread (2; row j + *threads is guarded against
 * gates*H), *nb batch rows per workgroup (1 | 4, the threshold of tn_dbg_rnn_route), *lds_fwd / *lds_bwd the dynamic LDS bytes of the
 * forward kernel and of the cell's BPTT kernel.  Refuses gates*H <= 1024 (tn_dbg_rnn_route answers for those) and > 2048.  Host
 * arithmetic only: touches no device. */
int tn_dbg_rnn_wide_route(int gates, int B, int H, int dirs, int *threads, int *rows, int *nb, int64_t *lds_fwd, int64_t *lds_bwd);
/* on = 1: every recurrent launch of the process (forward and BPTT) runs the wide kernels, also at gates*H <= 1024, where they give
 * the bits of the default kernels - which is what the hook is there to show; on = 0 (the default) restores the policy.  Process-wide,
 * not synchronised with launches in flight.  A test hook, not for production use: the wide kernels keep nothing of W_hh on chip. */
int tn_dbg_rnn_force_wide(int on);
/* *count: how many launches of the process took the wide recurrent kernels so far (forward and BPTT together), so that a test can tell
 * which family served a call. */
int tn_dbg_rnn_wide_launches(int64_t *count);

/* Which kernel families the fp16 DenseNet-121 encoder launches for an input size, create flags (0 | TN_ENC_EXACT_WEIGHTS; the TN_*
 * switches are read from the environment as tn_densenet121_create_ex reads them), a batch and a pass (calibrate: the layer-wise pass
 * of tn_densenet121_input_means): what tn_densenet121_profile would fill for such an encoder - name, launches, flops and bytes in
 * first-seen order, ms 0 - from the routing plan create and forward both follow (csrc/encoder_plan.h).  Refuses what create refuses
 * for the size and the flags, and TN_ENC_FP32 / TN_ENC_FP32X3, which are not planned.  Host arithmetic only: touches no device. */
int tn_dbg_encoder_plan(int height, int width, int flags, int batch, int calibrate, tn_kernel_stat *stats, int max_stats, int *n_stats);
/* The same plan for a forward that shares the chip with a neighbouring stream's call (a pipelined whole-batch call; never the
 * calibration pass): the same families, launches, flops and bytes, and *paired_out: how many of its steps take the paired launch
 * geometry of the 28x28 strip kernels (TN_NO_STRIP_PAIR, TN_STRIP_PAIR_MIN_BATCH; an even batch only). */
int tn_dbg_encoder_plan_shared(int height, int width, int flags, int batch, tn_kernel_stat *stats, int max_stats, int *n_stats,
                               int *paired_out);

/* The parameter table of a training handle, built by the function its create calls (csrc/param_table.h): one row per readable name,
 * in the order of the flat buffers.  where: 0 the flat parameter / gradient buffers (tn_*_buffers) at `offset` floats, 1 the
 * backbone's running-statistics buffer at `offset`, 2 a device buffer of its own (the "<bn>_batch_mean" / "_batch_var" test hooks;
 * offset 0).  The backbone's convolution weights sit in the flat buffers in (O, kh, kw, I) order.
 * which / dims / prefixes: TN_TRAINER_HEAD (gates, input, hidden, classes), rnn and dense prefix; TN_TRAINER_GNMT (gates, input,
 * hidden, embed, vocab, num_layers, num_bi_layers), the prefix, prefix_b ignored; TN_TRAINER_BACKBONE (classes, or 0 for the
 * backbone alone), backbone prefix and the classifier's (NULL with 0 classes).  Writes at most max_rows rows (rows NULL with
 * max_rows 0: count only); *n_rows the table's rows, *numel / *state_numel (optional) the floats of the flat buffers / of the
 * state buffer.  Host arithmetic only: touches no device. */
enum { TN_TRAINER_HEAD = 0, TN_TRAINER_GNMT = 1, TN_TRAINER_BACKBONE = 2 };
typedef struct tn_param_row {
  char name[96];
  int where;
  int64_t offset, count;
} tn_param_row;
int tn_dbg_trainer_params(int which, const int *dims, int n_dims, const char *prefix_a, const char *prefix_b, tn_param_row *rows,
                          int max_rows, int *n_rows, int64_t *numel, int64_t *state_numel);

/* One convolution of the fp32x3 encoder mode (csrc/dense_fp32x3.hip; which = 0) or, on the same operands, of the fp32 mode
 * (csrc/dense_fp32.hip; which = 1).  kind: 0 stem 7x7/2 (x: B frames in `layout`, H x W; epilogue relu(es y + et)), 1 dense 1x1,
 * 2 dense 3x3 (K = 1152, ldx = 128), 3 transition (2x2 average of relu(s x + t), then the 1x1); x an fp32 NHWC map (.., ldx), s / t
 * the BatchNorm applied on load (K values; 3x3: 128), es / et NULL except for the stem, y (M, ldy) fp32 written in columns
 * [yoff, yoff + N), M = B Ho Wo output pixels: all DEVICE, 16-byte aligned.  w_host: the GEMM's B operand (K, N) fp32, k-major
 * (stem k = c 49 + ky 7 + kx, 3x3 k = tap 128 + c), HOST; padded and - which = 0 - split and packed as tn_densenet121_create_ex
 * does.  tile, for either kernel: 0 the launcher's choice, 1 the small tile (1x1 / transition 128 x 64, 3x3 128 x 32), 2 the large one
 * (128 x 128, 3x3 256 x 32); the stem has one tile (128 x 64).  The selector's range, K a multiple of 32 (other than the stem's 147)
 * and the output window are the launchers' own refusals ("conv_fp32x3: ..." / "conv_fp32: ...").  Synchronous. */
int tn_dbg_conv_fp32x3(tn_ctx *ctx, int which, int kind, int tile, int layout, const void *x, int ldx, int K, const float *s, const float *t,
                       const float *w_host, int N, const float *es, const float *et, float *y, int ldy, int yoff, int64_t M, int H, int W,
                       int Ho, int Wo);

/* The fp32 mode's 3x3 stride-2 pad-1 max pool (csrc/dense_fp32.hip) on caller buffers: x (B, H, W, 64) fp32, y (B Ho Wo, ldy) fp32
 * written in columns [0, 64), Ho = (H - 1) / 2 + 1, Wo likewise, ldy >= 64 a multiple of 4: DEVICE, 16-byte aligned.  Synchronous. */
int tn_dbg_maxpool_fp32(tn_ctx *ctx, const float *x, int B, int H, int W, float *y, int ldy, int Ho, int Wo);

/* Tuning hook of the windowed recurrent kernel (csrc/rnn_window.hip): the samples one workgroup walks - 0 the library's choice,
 * 4, or twice the gates (6 GRU / 8 LSTM).  The results do not depend on it (scripts/bench_window_head.py measures both). */
int tn_dbg_window_head_rows_per_group(struct tn_window_head *h, int nb);

/* The sum of squares behind the global-norm clipping of the training steps (csrc/train.hip, grad_sumsq_kernel), run on caller
 * buffers: (dev, n) and (dev2, n2), DEVICE fp32, 4-byte aligned, any counts, either may be empty (NULL, 0).  *sumsq_host: the
 * sum as the finalize kernel holds it, in double.  Synchronous.  The layout the error bound of a test follows from: a grid of
 * TN_GRAD_SUMSQ_GRID workgroups of TN_GRAD_SUMSQ_BLOCK threads; the 16-byte-aligned body of a segment is cut into chunks of
 * TN_GRAD_SUMSQ_CHUNK floats, chunk c goes to workgroup c % GRID, and a thread adds CHUNK / BLOCK squares of a chunk to its fp32
 * partial serially; up to 3 floats before and 3 after the body go one each to threads of workgroup 0 (one more term per
 * segment); the BLOCK partials of a workgroup meet in an fp32 tree, the GRID results in double. */
#define TN_GRAD_SUMSQ_BLOCK 256
#define TN_GRAD_SUMSQ_CHUNK 4096
#define TN_GRAD_SUMSQ_GRID 1024
int tn_dbg_grad_sumsq(tn_ctx *ctx, const float *dev, int64_t n, const float *dev2, int64_t n2, double *sumsq_host);

/* The captioner's step kernels (csrc/gnmt_kernels.hip) on their own: each hook launches the production kernel on the ctx stream with
 * the grid, block and dynamic LDS the decoder / the training step compute for the shape, then synchronises.  All operands DEVICE
 * fp32 (valid_len / labels / tgt int32), 16-byte aligned; H % 4 == 0.  A null pointer (other than the optional ones), a pitch below
 * its width or a shape whose LDS passes the step kernels' 152 KiB is refused with TN_ERR_INVALID.
 * tn_dbg_gnmt_attention_fwd: transpose_bth_kernel on keyproj (B,T,H) row-major, then dec_attention_kernel<1> over R = B * beam rows
 * (row r belongs to clip r / beam): g0 (R,4H) the first cell's stacked pre-activations (GRU [r, z, n_i2h, n_h2h], LSTM [i, f, g, o]),
 * hprev (R rows of pitch ldh >= H), cprev (R,H; LSTM only, else NULL), mem (B,T,H), valid_len (B; clamped to [0, T]).  split_cap 0:
 * the split att_split picks; 16 / 8 / 4 / 2 / 1: min(pick, cap) - the LDS is sized for the split used.  Outputs: hn (R,H), cn (R,H;
 * LSTM only), x1 (R rows of pitch ldx1 >= 2H, columns [0, 2H) written: [h, context]), ctx_out (R,H), w_out (R,T). */
int tn_dbg_gnmt_attention_fwd(tn_ctx *ctx, const float *g0, const float *hprev, int ldh, const float *cprev, int lstm, const float *keyproj,
                              const float *mem, const int32_t *valid_len, int B, int T, int H, int beam, int split_cap, float *hn, float *cn,
                              float *x1, int ldx1, float *ctx_out, float *w_out);
/* trn_att_bwd_kernel: aw (B,T) the step's weights, mem / keyproj (B,T,H), d context = c0 + c1 (B rows of pitch lc0 / lc1 >= H; either
 * may be NULL, not both) -> ds (B,T), dctx (B,H), dh0 (B,H). */
int tn_dbg_gnmt_attention_bwd(tn_ctx *ctx, const float *aw, const float *mem, const float *keyproj, const float *c0, int lc0, const float *c1,
                              int lc1, const int32_t *valid_len, int B, int T, int H, float *ds, float *dctx, float *dh0);
/* trn_att_outer_kernel: aw / ds (steps,B,T), dctx (steps,B,H), h0 (steps * B rows of pitch ldh >= H) -> dmem, dkp (B,T,H). */
int tn_dbg_gnmt_attention_outer(tn_ctx *ctx, const float *aw, const float *ds, const float *dctx, const float *h0, int ldh, int steps, int B,
                                int T, int H, float *dmem, float *dkp);
/* trn_ce_bwd_kernel + the column sum of its loss rows, and masked_ce_kernel on the same operands: logits (B,L,V), labels (B rows of
 * pitch ld >= L), valid_len (B) -> dlogits (L,B,V), loss_rows (L,B), loss (1: the token-averaged loss), masked_loss (B: the
 * per-sample mean over L of the masked negative log-probability). */
int tn_dbg_gnmt_ce(tn_ctx *ctx, const float *logits, const int32_t *labels, int ld, const int32_t *valid_len, int B, int L, int V,
                   float *dlogits, float *loss_rows, float *loss, float *masked_loss);
/* trn_emb_grad_kernel: dx0 (L,B,K0) step-major with K0 > E (the first E columns are read), tgt (B rows of pitch ld >= L; an id <= 0
 * counts as row 0) -> demb (V,E), every row assigned. */
int tn_dbg_gnmt_emb_grad(tn_ctx *ctx, const float *dx0, int K0, const int32_t *tgt, int ld, int B, int L, int E, int V, float *demb);
/* One launch of dec_beam_kernel<NBM> (the last launch of a beam-search step) over B clips of `beam` rows, R = B * beam, with the
 * instantiation, dynamic LDS, projection split and extra workgroups tn_gnmt_beam_search computes for the shape.  split_cap as in
 * tn_dbg_gnmt_attention_fwd.  Refused: a null pointer that is not optional, H % 4 != 0, a pitch below its width, beam outside
 * 1..16, V < beam, LDS past 152 KiB, misaligned operands of the p0 tiles.
 *   g1 (R,4H) the last cell's stacked pre-activations; x1 the cell's step input [input (2H) | h_prev (H)]: row-major with pitch
 *   ldx1 >= 3H, or (ldx1 < 0) k-group-major with -ldx1 >= R rows, element (r, k) at ((k / 4) * (-ldx1) + r) * 4 + k % 4; c1cur (R,H; LSTM,
 *   else NULL); wp_host (V,H) / bp_host (V; NULL: no bias) HOST, packed as tn_gnmt_create packs tgt_proj; scores / alive / vlen (R) in
 *   and out; bp_par / bp_word (step,R): row step - 1 is written; any_alive (1): or-ed with 1 when a row stays alive; hstate (R,H) or
 *   NULL: the residual form (the projection sees h + x1[:, 0:H]); parent_out (R) or NULL.
 *   Token form (tok_out (R) != NULL): the words go to tok_out; with p0 (R,4H) != NULL, extra workgroups compute
 *   p0 = x1[:, 0:2H] . w1x[:, 0:2H]^T + b1x (w1x (4H rows of pitch K1p), b1x (4H)) beside the clips; p0 = w1x = b1x = NULL: none.
 *   x0 form (tok_out NULL): x0 (R, E + 2H) = [emb[word] (emb (V,E)), ctxv[parent], h0n[parent]] (both (R,H)), c0cur = c0n[parent] (LSTM).
 *   Always: x1[:, 2H:3H] = h[parent] (hstate's rows in the residual form), c1cur = c[parent] (LSTM). */
int tn_dbg_gnmt_beam_step(tn_ctx *ctx, const float *g1, float *x1, int ldx1, int lstm, float *c1cur, const float *wp_host,
                          const float *bp_host, int B, int H, int E, int V, int beam, int step, float lp, float prev_lp, int eos,
                          int split_cap, float *scores, int32_t *alive, int32_t *vlen, int32_t *bp_par, int32_t *bp_word,
                          int32_t *any_alive, float *hstate, int32_t *parent_out, int32_t *tok_out, const float *w1x, const float *b1x,
                          int K1p, float *p0, const float *emb, const float *ctxv, const float *h0n, const float *c0n, float *x0,
                          float *c0cur);
/* The latency GEMM (csrc/linear.h lat_tile_f32) through its launchers: Y (M rows of pitch ldy >= N) = X W^T + bias, W (N rows of
 * pitch ldw >= K) row-major, bias (N) or NULL, all DEVICE.  form 0: launch_linear_f32_lat2 - X row-major (pitch ldx >= K); the
 * columns from nsplit (a multiple of 16; >= N: none) contract only k < K2.  form 1: launch_linear_f32_lat_wk4 on the k-group-major
 * copy of W built here; X row-major, or (ldx < 0) k-group-major with -ldx >= M rows, element (m, k) at ((k / 4) * (-ldx) + m) * 4 + k % 4;
 * needs K % 4 == 0, ldx % 4 == 0 and a 16-byte aligned X.  *route (optional): 0 the latency kernel, 1 its k-group-major form, 2 the
 * launch_linear_f32 fallback (form 0 with K < 128, operands off float4 alignment or more than 4096 tiles).  Synchronous. */
int tn_dbg_linear_lat(tn_ctx *ctx, int form, const float *X, int ldx, const float *W, int ldw, const float *bias, float *Y, int ldy, int M,
                      int N, int K, int nsplit, int K2, int *route);

#ifdef __cplusplus
}
#endif
#endif /* TENNIS_HIP_DEBUG_H */
