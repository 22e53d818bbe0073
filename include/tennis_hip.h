/*
 * tennis_hip.h — C ABI of libtennis_hip.so: the MI355X (gfx950) hot path of
 * HaydenFaulkner/Tennis, hand-written HIP behind the reference's model surface.
 *
 * The reference has NO FFI boundary of its own (pure Python on MXNet,
 * SURVEY §8b).  Each entry point below replaces the device work that one
 * reference call performs inside MXNet; the cited file:line is the reference
 * call site that a maintainer would re-point at this library (INTEGRATION.md
 * shows the ctypes stub).
 *
 * Conventions
 *   - every function returns 0 on success, a negative tn_status otherwise;
 *     tn_last_error() gives a thread-local message for the last failure;
 *   - all tensor pointers are DEVICE pointers on the ctx's device unless the
 *     parameter name ends in _host; the caller owns every input/output buffer;
 *     the library owns weights and workspace inside opaque handles;
 *   - calls on one tn_ctx are ordered on its HIP stream and asynchronous;
 *     tn_ctx_sync() waits.  A ctx is not re-entrant; use one ctx per thread.
 *   - no allocation happens in *_forward.
 */
#ifndef TENNIS_HIP_H
#define TENNIS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  TN_OK = 0,
  TN_ERR_INVALID = -1,   /* bad argument / shape (mirrors the reference's asserts) */
  TN_ERR_HIP = -2,       /* HIP runtime error */
  TN_ERR_MISSING = -3,   /* a required parameter name was not supplied */
  TN_ERR_NOMEM = -4
} tn_status;

/* Input frame layouts accepted by tn_densenet121_forward. */
typedef enum {
  TN_LAYOUT_NCHW_F32 = 0, /* reference layout: ToTensor+Normalize output (evaluate.py:96-97) */
  TN_LAYOUT_NHWC_F16 = 1, /* native: normalised frames, fp16, 3 channels */
  TN_LAYOUT_NHWC_U8 = 2   /* decoded RGB bytes; ToTensor+Normalize fused into the stem load */
} tn_layout;

typedef enum { TN_RNN_GRU = 0, TN_RNN_LSTM = 1 } tn_rnn_kind;
typedef enum { TN_POOL_MAX = 0, TN_POOL_MEAN = 1 } tn_pool_kind;

/* A named host tensor (Gluon parameter name -> fp32 data). */
typedef struct {
  const char *name;
  const float *data_host;
  int64_t numel;
} tn_param;

typedef struct tn_ctx tn_ctx;
typedef struct tn_encoder tn_encoder;
typedef struct tn_dense tn_dense;
typedef struct tn_birnn tn_birnn;
typedef struct tn_gnmt tn_gnmt;

int tn_version(void);
const char *tn_last_error(void);

/* ---- context: one per (device, stream) --------------------------------- */
/* `stream` is the hipStream_t to launch on (e.g. torch's current stream; NULL is
 * HIP's default stream).  With own_stream != 0 the library creates and owns a
 * non-blocking stream instead and `stream` is ignored.  Replaces: mx.gpu(i)
 * context selection, reference evaluate.py:85. */
int tn_ctx_create(int device, void *stream, int own_stream, tn_ctx **out);
void *tn_ctx_stream(tn_ctx *ctx);
int tn_ctx_sync(tn_ctx *ctx);       /* replaces the implicit sync of .asnumpy(), evaluate.py:314 */
int tn_ctx_destroy(tn_ctx *ctx);

/* ---- frame encoder: DenseNet-121 .features ------------------------------ */
/* Replaces get_model('DenseNet121', pretrained=True).features (reference
 * evaluate.py:125, train.py:204, train_gnmt.py:150) and its forward
 * net.backbone(x) (evaluate.py:313).  `params` are Gluon-named fp32 host
 * tensors "<prefix>conv0_weight", "<prefix>stage1_batchnorm0_gamma", ...
 * (H,W) is the input size (224 or 512 in the reference), feature_dim is
 * 1024*floor(H/32/7)*floor(W/32/7) (1024 @224, 4096 @512; train.py:259). */
int tn_densenet121_create(tn_ctx *ctx, const tn_param *params, int n_params, const char *prefix,
                          int height, int width, int max_batch, tn_encoder **out);
/* The same with flags.  TN_ENC_EXACT_WEIGHTS: the fp32 convolution weights of the dense layers and transitions are
 * kept as two fp16 numbers each (hi + lo, 22 bits of the fp32 weight) and every product is formed with both: features
 * within 1e-3 of the fp32 reference evaluated on the UN-rounded weights (reference models/vision/definitions.py:27-33
 * evaluates fp32 parameters), at twice the MFMA work of those layers.  Without the flag the weights are rounded to
 * fp16 once (the served fp16 model).  Any input size since round 6 (maps no fused kernel tiles run their layers un-fused with the
 * same hi + lo pass; flat frames at 448 x 448 / 512 x 512 keep a tail of 1.2e-3 that is the fp16 activation path's: DESIGN.md section 4). */
#define TN_ENC_EXACT_WEIGHTS 1
/* TN_ENC_FP32: the reference's own evaluation - fp32 parameters evaluated in fp32 (models/vision/definitions.py:27-33) - for
 * any checkpoint.  Every activation is stored in fp32 and every product is formed in fp32 on the f32-input MFMA (exact f32,
 * a k-ordered fma chain); the weights are the raw fp32 parameters (no fp16 conversion, no hi + lo split), the BatchNorms are
 * folded in double and rounded to fp32 once.  Features within 1e-3 of the fp32 reference on every frame family, seeded and
 * trained-looking parameters, every input size, at the f32 matrix rate (1/16 of fp16).  Its own kernels
 * (csrc/dense_fp32.hip) and its own fp32 workspace; every input layout, any batch up to max_batch, pipelined forwards and
 * the per-family profile (families "fp32_*").  tn_densenet121_input_means and tn_densenet121_read_tap refuse such an encoder.
 * TN_ENC_FP32 | TN_ENC_EXACT_WEIGHTS selects this mode as well. */
#define TN_ENC_FP32 4
/* TN_ENC_FP32X3: the fp32 mode's network - fp32 activation maps, fp32 accumulators, the same folds, workspace, layouts, batches,
 * pipelining - with the products on the bf16 matrix pipe (csrc/dense_fp32x3.hip): every fp32 operand is handed over as three
 * bf16 terms (v1 = bf16(v), v2 = bf16(v - v1), v3 = bf16(v - v1 - v2), 24 bits between them, fp32's exponent range: no scaling,
 * no calibration, any checkpoint) and the six largest of the nine cross products are formed per 16-wide k-step, in a fixed order.
 * The dropped products are below 2^-24 |a||b|: the result is an fp32 accumulation that differs from the fp32 mode's in summation
 * grouping only, and holds the same 1e-3 bar.  Profile families "fp32x3_*"; tn_densenet121_input_means and
 * tn_densenet121_read_tap refuse such an encoder.  TN_ENC_FP32X3 | TN_ENC_EXACT_WEIGHTS selects this mode as well;
 * TN_ENC_FP32X3 | TN_ENC_FP32 is refused (two modes). */
#define TN_ENC_FP32X3 8
/* The three-term split of the fp32x3 mode on the host (no GPU involved): t1 + t2 + t3 reproduces w to 2^-24 |w|, every term the
 * bit pattern of a bf16 number (round to nearest even). */
int tn_fp32x3_split(const float *w, int64_t n, uint16_t *t1, uint16_t *t2, uint16_t *t3);
int tn_densenet121_create_ex(tn_ctx *ctx, const tn_param *params, int n_params, const char *prefix, int height, int width,
                             int max_batch, int flags, tn_encoder **out);
int tn_densenet121_feature_dim(const tn_encoder *enc);
size_t tn_densenet121_workspace_bytes(const tn_encoder *enc);
/* x: `batch` frames in `layout`; feat: (batch, feature_dim) fp32, NCHW-flatten order. */
int tn_densenet121_forward(tn_encoder *enc, const void *x, tn_layout layout, int batch, float *feat);
/* The same forward, and the class activation maps of a Dense(feature_dim -> units) behind it.  The network ends in
 * BN -> ReLU -> AvgPool2D(7) -> Flatten -> Dense, so a logit is a sum over the cells of the last map and the maps need no backward
 * pass: with A = relu(bn(map)) as the head averages it,
 *   maps[b,c,y,x] = (1/49) sum_k W[c, k PH PW + (y/7) PW + (x/7)] A[b,k,y,x],    logit[b,c] = bias[c] + sum_{y,x} maps[b,c,y,x].
 * Same contract as tn_densenet121_forward (layouts, max_batch, pipelining and join: the maps are ordered exactly as the
 * features are); features are bit-identical to that call's.  maps: (batch, units, h, w) fp32 on the DEVICE, h x w from
 * tn_densenet121_class_map_dims (7 x 7 at 224^2, 14 x 14 at 512^2: the 16 x 16 map's rows / columns 14 and 15 are dropped by
 * the pool and belong to no cell).  The maps are computed from the map the head reads in that forward, in every mode, in a
 * fixed order: bit-reproducible, and independent of how the batch was split.  classes->in_units must be the feature width,
 * units <= 64, and the Dense must belong to the encoder's context; refused otherwise (tn_last_error names the argument). */
int tn_densenet121_forward_class_maps(tn_encoder *enc, const void *x, tn_layout layout, int batch, float *feat,
                                      const tn_dense *classes, float *maps);
int tn_densenet121_class_map_dims(const tn_encoder *enc, int *h, int *w);        /* 7 PH, 7 PW */
/* Pipelined forwards.  A large batch runs as two half batches on two library-owned streams; by default forward makes
 * the ctx's stream wait for both before it returns, so the call is stream-ordered like every other one.  With
 * set_pipelined(enc, 1) forward does NOT: consecutive forwards then overlap (the first half of call i+1 starts beside
 * the tail of the second half of call i, which runs on half of the CUs), and the CALLER orders the results:
 * tn_densenet121_join(enc, 0) makes the ctx's stream wait for the last forward, join(enc, 1) for the one before it
 * (results consumed one call behind).  Until its join, a forward's input x must not be overwritten and its feat not
 * read; set_pipelined(enc, 0) joins everything outstanding.  Replaces nothing in the reference (MXNet's engine
 * overlaps independent ops by itself); it exists for streaming a corpus through the encoder (config C4).
 * (Round 6: from 128 frames per call on, a pipelined forward runs its WHOLE batch on one of the two streams, consecutive calls
 * alternating, each in its own workspace set - at most two forwards are in flight, as before; same results bit for bit,
 * same join contract; TN_NO_INTERLEAVE=1 in the environment keeps the half-batch form.) */
int tn_densenet121_set_pipelined(tn_encoder *enc, int on);
int tn_densenet121_join(tn_encoder *enc, int lag);
/* Calibration statistics for the calibrated fp16 conversion (tennis_amd/weights.py::as_fp16_model(input_means=...)):
 * `batch` frames go through the layer-wise kernels, and for each of the 119 convolutions behind the stem, in execution order
 * (per dense layer the 1x1's K input channels, then the 3x3's 128; a transition's inputs after its block), the mean over all
 * pixels of the OPERAND that convolution's folded weights multiply is written to means_host (fp32, *numel values): for a dense
 * layer's 1x1 the clamped stored activation clamp(x, lo, hi) (tn_bn_relu_clamp_fold; relu(bn(x)) = sw * that + tc; exactly 0 in a
 * channel the fold made a constant, lo == hi), for its 3x3
 * the ReLU'd bottleneck, for a transition relu(bn(x)).  (The stem's operand mean, x - 255 mean_c, is a property of the frame and
 * is computed by the caller.) */
int tn_densenet121_input_means(tn_encoder *enc, const void *x, tn_layout layout, int batch, float *means_host,
                               int64_t capacity, int64_t *numel);
/* Host side of that conversion (no GPU involved; csrc/calib_host.hip): w (N, K) fp32 -> out (N, K), every entry one of the two
 * fp16 neighbours of w's entry, chosen per output row so that the row's rounding error is (nearly) orthogonal to all F rows of
 * A (F, K) - the per-frame mean input activations of F calibration frames (one tn_densenet121_input_means call per frame) -
 * by a greedy pass and `sweeps` passes of coordinate descent on || A d ||^2 / F + ridge * sum_k (d[k] rms_f A[f][k])^2.
 * The reference evaluates fp32 parameters (models/vision/definitions.py:27-33): this keeps ONE fp16 number per weight within
 * the 1e-3 bar of that evaluation. */
int tn_round_fp16_calibrated(const float *w, int rows, int cols, const double *A, int frames, int sweeps, double ridge, float *out);
/* The `.npy` side of `evaluate.py --save_feats` (reference evaluate.py:306-321: np.save(feat_path, feat[i]) per frame unless the file
 * exists): a pool of host threads that creates the directories and writes one NumPy-format-1.0 float32 file per row, byte for byte
 * what np.save writes.  submit copies the rows (host memory) and returns; drain waits for everything submitted, returns the totals
 * since creation and fails with the first file error.  Host code, no GPU involved (csrc/npy_host.hip). */
typedef struct tn_npy_writer tn_npy_writer;
int tn_npy_writer_create(int threads, tn_npy_writer **out);
int tn_npy_writer_submit(tn_npy_writer *w, const float *rows_host, int n, int dim, const char *const *paths, int skip_existing);
int tn_npy_writer_drain(tn_npy_writer *w, int64_t *written, int64_t *skipped);
int tn_npy_writer_destroy(tn_npy_writer *w);
/* BatchNorm -> ReLU in front of a dense layer's 1x1 convolution (gluoncv DenseNet _make_dense_layer, reference call site
 * models/vision/definitions.py:30) in the fused kernels' rounding-free form: relu(scale x + shift) = sw clamp(x, lo, hi) + tc with
 * lo / hi fp16 numbers (the ReLU threshold -shift / scale on the side the scale's sign says, +-65504 on the other); sw[k]
 * multiplies column k of the 1x1 weights before they are rounded to fp16 - part of how the fp16 model is defined
 * (weights.as_fp16_model calls this so that the host and the library agree bit for bit) - and sum_k w[n][k] tc[k] joins the shift
 * of the BatchNorm behind the convolution.  Host code, no GPU involved (csrc/calib_host.hip). */
int tn_bn_relu_clamp_fold(const float *gamma, const float *beta, const float *running_mean, const float *running_var, int channels,
                          float *lo, float *hi, float *sw, float *tc);
int tn_densenet121_destroy(tn_encoder *enc);

/* ---- nn.Dense(units, flatten=True) -------------------------------------- */
/* Replaces FrameModel.classes / CNNRNN.classes (reference
 * models/vision/definitions.py:25,32,101,108-109).  y = x W^T + b, fp32. */
int tn_dense_create(tn_ctx *ctx, const float *weight_host, const float *bias_host, int units,
                    int in_units, tn_dense **out);
int tn_dense_forward(tn_dense *d, const float *x, int rows, float *y);
/* Temporal activation maps of a head that ends in max over T -> this Dense (CNNRNN, TemporalPooling(pool="max"): reference
 * models/vision/definitions.py:66-69,106-109; the maps themselves have no counterpart there).  pooled (batch, in_units) fp32 is what
 * the Dense saw, steps (batch, in_units) int32 the window position in [0, window) each unit's maximum was read from
 * (tn_temporal_pool_arg and the *_arg / *_tam calls below), tam (batch, units, window) fp32:
 *   tam[b][c][t] = sum over { k : steps[b][k] == t }, k ascending, of weight[c][k] * pooled[b][k],
 * so bias[c] + sum_t tam[b][c][t] is the logit of tn_dense_forward in real arithmetic.  Every entry is written, a step no unit names
 * is 0.0f, a steps entry outside [0, window) contributes nothing and is never used as an address.  No atomics: a sample's maps do
 * not depend on the batch it is in.  All DEVICE buffers.  A recurrent state at step t has seen the steps before it (after it, in the
 * reverse direction): the maps say which step's STATE a logit was read from, not which single frame caused it.
 * Nulls, batch < 1 and window < 1 are TN_ERR_INVALID.  Does not allocate. */
int tn_dense_step_maps(tn_dense *d, const float *pooled, const int32_t *steps, int batch, int window, float *tam);
int tn_dense_destroy(tn_dense *d);

/* ---- gluon.rnn.GRU/LSTM(hidden, layout='NTC', bidirectional=True) ------- */
/* Replaces CNNRNN.rnn (reference models/vision/definitions.py:94-96,106) and
 * one bidirectional layer of GNMTEncoder (models/captioning/gnmt.py:141-148).
 * params: "<prefix>{l,r}0_{i2h,h2h}_{weight,bias}"; gate order GRU [r,z,n],
 * LSTM [i,f,g,o].  x (B,T,F) fp32 -> seq (B,T,2H) fp32 = concat(fwd,bwd);
 * zero initial state.  valid_len (B,) int32 or NULL: steps >= valid_len are
 * skipped and emit zeros; the reverse direction starts at valid_len-1.
 * h_last/c_last (2,B,H) fp32 or NULL receive the final states [fwd,bwd].
 * hidden % 4 == 0 and gates*hidden <= 2048 (gates 3 GRU / 4 LSTM: GRU up to 680, LSTM up to 512); past gates*hidden = 1024
 * the recurrence runs two gate rows per thread and streams W_hh every step (docs/kernels.md). */
int tn_birnn_create(tn_ctx *ctx, tn_rnn_kind kind, int input_size, int hidden, const tn_param *params,
                    int n_params, const char *prefix, int bidirectional, int max_rows, tn_birnn **out);
int tn_birnn_forward(tn_birnn *r, const float *x, int batch, int steps, const int32_t *valid_len,
                     float *seq, float *h_last, float *c_last);
int tn_birnn_destroy(tn_birnn *r);

/* ---- test transform, geometric half: Resize + CenterCrop on decoded frames ----- */
/* Replaces transforms.Resize(data_shape + 32) + transforms.CenterCrop(data_shape) of the reference's
 * transform_test (evaluate.py:93-96; gluon Resize -> mx.image.imresize interp=1 = cv::resize INTER_LINEAR on
 * 8-bit RGB [EXT]; CenterCrop offset int((s - c) / 2)).  src (batch, src_h, src_w, 3) uint8 RGB, dst
 * (batch, crop, crop, 3) uint8 = TN_LAYOUT_NHWC_U8 for tn_densenet121_forward, whose stem load applies
 * ToTensor + Normalize (evaluate.py:96-97).  Both DEVICE buffers; bit-exact integer arithmetic. */
typedef struct tn_preproc tn_preproc;
int tn_preproc_create(tn_ctx *ctx, int src_h, int src_w, int resize, int crop, tn_preproc **out);
int tn_preproc_forward(tn_preproc *p, const uint8_t *src, int batch, uint8_t *dst);
int tn_preproc_destroy(tn_preproc *p);
/* Train-time augmentation of the frame classifier (reference train.py:127-136: transforms.RandomResizedCrop(data_shape),
 * RandomFlipLeftRight(), RandomColorJitter(brightness, contrast, saturation), RandomLighting(alpha) in front of ToTensor / Normalize):
 * the image arithmetic for a batch, one parameter record per frame.  The random draws are the caller's (MXNet's generator cannot be
 * reproduced: tennis_amd/transforms.py draws them the way mx.image.random_size_crop / the image_random operators do).  src (batch,
 * src_h, src_w, 3) uint8 RGB and every other buffer on the device, frames_host = the same records on the host (validated there);
 * tmp batch * size * size * 3 bytes, gray_tmp batch floats; dst (batch, size, size, 3) uint8 - what ToTensor receives. */
typedef struct tn_aug_frame {
  int32_t x0, y0, cw, ch;        /* crop window (random_size_crop), resized to size x size with cv::resize(INTER_LINEAR) */
  int32_t flip;                  /* RandomFlipLeftRight */
  int32_t order;                 /* four 2-bit fields, first applied in the low bits: 0 brightness, 1 contrast, 2 saturation, 3 hue (= nothing) */
  float brightness, contrast, saturation;   /* the operators' alphas: 1 + U(-p, p) */
  float light[3];                /* RandomLighting: eigvec (alpha * eigval), per channel */
} tn_aug_frame;
int tn_augment_forward(tn_ctx *ctx, const uint8_t *src, int batch, int src_h, int src_w, const tn_aug_frame *frames_dev,
                       const tn_aug_frame *frames_host, int size, uint8_t *tmp, float *gray_tmp, uint8_t *dst);
/* ToTensor + Normalize (reference evaluate.py:96-97, train.py:138-139) for consumers of fp32 frames (the fine-tuning
 * step; the inference encoder fuses it into its stem load): dst[p][c] = (src[p][c] / 255 - mean[c]) / std[c],
 * in float32 with two divisions, each operation rounded once (dataset.default_transform's formula bit for bit).
 * src (pixels, 3) uint8 NHWC, dst (pixels, 3) float NHWC, both DEVICE; mean3 / std3 HOST arrays of 3 floats, no std zero.
 * src may start at any byte and dst at any float: the 12-bytes-in / three-float4-out path is taken when src is 4-byte
 * and dst 16-byte aligned, a byte-wise loop otherwise, with the same values. */
int tn_to_tensor_normalize(tn_ctx *ctx, const uint8_t *src, long pixels, const float *mean3, const float *std3, float *dst);

/* ---- JPEG decode on the device ------------------------------------------------ */
/* Replaces mx.image.imread(path, 1) of the reference's frame loader (dataset.py:204,216: OpenCV imdecode -> libjpeg
 * with its default parameters, JDCT_ISLOW and fancy upsampling) for a batch of files of ONE geometry (the frames of
 * a video): baseline / extended sequential Huffman JPEG (SOF0, SOF1), 8 bit, one interleaved scan, grey or YCbCr
 * 4:4:4 / 4:2:2 / 4:2:0, restart intervals included.  data_host[i] / sizes[i]: the i-th file's bytes in HOST memory;
 * rgb: DEVICE buffer (n, height, width, 3) uint8 RGB = the src of tn_preproc_forward (grey files are replicated to
 * three channels, as imread flag=1 does).  Only the marker segments are read on the host; Huffman decoding
 * (parallel inside each file), IDCT, upsampling and colour conversion run on the device, bit-exact with libjpeg's
 * integer arithmetic.  Anything else (progressive, arithmetic coding, 12 bit, CMYK, multi-scan, files of different
 * geometry in one call, corrupt data) is refused with TN_ERR_INVALID and a message naming the file.  The call
 * synchronises the ctx's stream (it reads back the convergence flag of the parallel Huffman decoder) and may grow
 * the handle's workspace.  tn_jpeg_info parses one file's header on the host (no device work). */
typedef struct tn_jpeg tn_jpeg;
int tn_jpeg_create(tn_ctx *ctx, tn_jpeg **out);
int tn_jpeg_info(const uint8_t *data_host, size_t size, int *width, int *height, int *components, int *h_samp, int *v_samp);
int tn_jpeg_decode(tn_jpeg *j, const uint8_t *const *data_host, const size_t *sizes, int n, uint8_t *rgb, int *width, int *height);
int tn_jpeg_destroy(tn_jpeg *j);

/* ---- F.max / F.mean over axis 1 ------------------------------------------ */
/* Replaces reference models/vision/definitions.py:66-69,107.  x (B,T,F) -> y (B,F). */
int tn_temporal_pool(tn_ctx *ctx, const float *x, int batch, int steps, int feat, tn_pool_kind kind,
                     float *y);
/* F.max over axis 1 (definitions.py:66-69,107) with the position of every maximum: y (B,F) as TN_POOL_MAX above, arg (B,F) int32 the
 * smallest t that holds it (the position the training step routes the gradient to). */
int tn_temporal_pool_arg(tn_ctx *ctx, const float *x, int batch, int steps, int feat, float *y, int32_t *arg);

/* ---- dense windowed evaluation of the temporal heads ------------------------ */
/* Replaces the evaluation loop of reference evaluate.py:274-303 for `--feats_model M --window W --temp_pool gru|lstm`
 * (model 0042): TennisSet.__getitem__ loading the W feature files of every sample (dataset.py:190-201,206-213), the
 * loader stacking them to (B, W, F), and CNNRNN.forward in feature mode (models/vision/definitions.py:94-96,106-109:
 * bi-GRU / bi-LSTM -> F.max(axis=1) -> Dense).  Here the (rows, F) feature matrix stays on the device, its i2h projection
 * runs once per row (project), and forward gathers every sample's window inside the recurrent kernel: step t of sample b
 * reads row clamp(centre[b] + (t - window/2) * stride, lo[b], hi[b]) - dataset.py:190-201 in units of matrix rows, the
 * offsets range(int(-w/2), ceil(w/2)) - clamped once more to [0, rows-1], so no content of the index arrays reads outside.
 * Neither (samples, W, F) nor the (samples, W, 2H) sequence is materialised.  Parameters as tn_head_create.
 * project: feats (rows, F) fp32 DEVICE, rows <= max_rows; one project serves any number of forward calls.
 * forward: centre / lo / hi (samples,) int32 DEVICE, samples <= max_samples; pooled (samples, 2H) fp32 or NULL, logits
 * (samples, classes) fp32, DEVICE.  forward before project, nulls, rows / samples over the handle's limits and window or
 * stride < 1 are TN_ERR_INVALID.  Neither call allocates.
 * The windowed recurrent kernel keeps one gate row per thread: gates*hidden <= 1024 here (GRU 340, LSTM 256), not the 2048 of
 * tn_birnn_create / tn_head_create; dense windowed evaluation of a wider head is refused at create. */
typedef struct tn_window_head tn_window_head;
int tn_window_head_create(tn_ctx *ctx, tn_rnn_kind kind, int input_size, int hidden, int classes, const tn_param *params,
                          int n_params, const char *rnn_prefix, const char *dense_prefix, int max_rows, int max_samples,
                          tn_window_head **out);
int tn_window_head_project(tn_window_head *h, const float *feats, int rows);
int tn_window_head_forward(tn_window_head *h, const int32_t *centre, const int32_t *lo, const int32_t *hi, int samples,
                           int window, int stride, float *pooled, float *logits);
/* forward over a row TABLE instead of (centre, lo, hi): the evaluation loop of reference evaluate.py:274-303 for a split whose
 * windows (dataset.py:190-201) have no arithmetic form - thinned-out or scattered samples, a stride that is no multiple of
 * `every`, window frames that are no sample (TennisSet.window_table) - and for CNNRNN on frames (definitions.py:104-109), whose
 * rows the model's own backbone produced.  idx (samples, window) int32 DEVICE, row-major: step t of sample b reads row
 * clamp(idx[b * window + t], 0, rows-1) of the projected matrix, unconditionally; a negative entry is row 0, not a zero row.
 * Runs after tn_window_head_project, with the limits and errors of tn_window_head_forward (samples <= max_samples, fewer than
 * 2^30 table entries); a table that spells out a (centre, lo, hi, stride) window gives that call's bits.  Does not allocate. */
int tn_window_head_forward_rows(tn_window_head *h, const int32_t *idx, int samples, int window, float *pooled /* may be NULL */,
                                float *logits);
/* tn_window_head_forward / tn_window_head_forward_rows (the evaluation loop of reference evaluate.py:274-303 over
 * definitions.py:106-109) that also say where each logit was read from: steps (samples, 2H) int32 or NULL, the window position t in
 * [0, window) of every pooled unit's maximum - the smallest such t, in both directions - and tam (samples, classes, window) fp32, the
 * maps of tn_dense_step_maps for the handle's own Dense.  pooled and logits are the bits of the calls without maps; a table that
 * spells out a (centre, lo, hi, stride) window gives the arithmetic form's steps and tam.  The limits and errors of the calls they
 * extend, tam NULL included.  With steps == NULL the handle allocates a (max_samples, 2H) int32 buffer at the first such call and
 * nothing afterwards; a handle that never asks allocates nothing. */
int tn_window_head_forward_tam(tn_window_head *h, const int32_t *centre, const int32_t *lo, const int32_t *hi, int samples,
                               int window, int stride, float *pooled /* may be NULL */, float *logits,
                               int32_t *steps /* may be NULL */, float *tam);
int tn_window_head_forward_rows_tam(tn_window_head *h, const int32_t *idx, int samples, int window, float *pooled /* may be NULL */,
                                    float *logits, int32_t *steps /* may be NULL */, float *tam);
int tn_window_head_destroy(tn_window_head *h);
/* TemporalPooling.forward in feature mode over the same windows (definitions.py:66-69 on the (B, W, F) batch of
 * dataset.py:190-213): feats (rows, feat) -> y (samples, feat), max or mean over the window's gathered rows. */
int tn_temporal_pool_windows(tn_ctx *ctx, const float *feats, int rows, int feat, const int32_t *centre, const int32_t *lo,
                             const int32_t *hi, int samples, int window, int stride, tn_pool_kind kind, float *y);
/* ... and over a row table (definitions.py:66-69 on the batch of dataset.py:190-201 for any split layout, and for
 * TemporalPooling on frames, evaluate.py:242-244): y[b] = max / mean over t ascending of row clamp(idx[b * window + t], 0,
 * rows-1); idx (samples, window) int32 DEVICE.  The bits of tn_temporal_pool_windows on a table that spells out its windows. */
int tn_temporal_pool_rows(tn_ctx *ctx, const float *feats, int rows, int feat, const int32_t *idx, int samples, int window,
                          tn_pool_kind kind, float *y);
/* The max pool of the two calls above (definitions.py:66-67 on the same windows) with arg (samples, feat) int32: the smallest window
 * position whose row holds the maximum.  y is TN_POOL_MAX's, bit for bit. */
int tn_temporal_pool_windows_arg(tn_ctx *ctx, const float *feats, int rows, int feat, const int32_t *centre, const int32_t *lo,
                                 const int32_t *hi, int samples, int window, int stride, float *y, int32_t *arg);
int tn_temporal_pool_rows_arg(tn_ctx *ctx, const float *feats, int rows, int feat, const int32_t *idx, int samples, int window,
                              float *y, int32_t *arg);

/* ---- temporal-head training step ------------------------------ */
/* bi-GRU / bi-LSTM(hidden) (`kind`; CNNRNN type='gru'|'lstm', definitions.py:93-96; LSTM gates [i,f,g,o]) over
 * features -> max over T -> Dense(classes) -> SoftmaxCrossEntropyLoss, backward, SGD with
 * momentum and weight decay: the frozen-backbone recipe of reference train.py (gluon.Trainer(..., 'sgd', {lr,
 * momentum, wd}) :298-299; SoftmaxCrossEntropyLoss :324; ag.record / ag.backward / trainer.step(batch_size)
 * :410-424) on the CNNRNN model of models/vision/definitions.py:94-110 in feature mode.
 * Parameters use the Gluon names (<rnn_prefix>{l0,r0}_{i2h,h2h}_{weight,bias}, <dense_prefix>{weight,bias}).
 * forward_backward leaves d(sum of per-sample losses)/d(param) in the gradient buffer; the caller may all-reduce
 * that buffer over ranks (tn_head_buffers gives the flat device arrays) before tn_head_sgd_step, whose update is
 * MXNet's sgd_mom_update: mom = momentum*mom - lr*(rescale_grad*grad + wd*w); w += mom.
 * hidden % 4 == 0 and gates*hidden <= 2048, as tn_birnn_create. */
typedef struct tn_head tn_head;
int tn_head_create(tn_ctx *ctx, tn_rnn_kind kind, int input_size, int hidden, int classes, const tn_param *params,
                   int n_params, const char *rnn_prefix, const char *dense_prefix, int max_batch, int max_steps, tn_head **out);
int tn_head_forward_backward(tn_head *h, const float *x, const int32_t *labels, int batch, int steps, float *loss,
                             float *logits);
/* The same step from a device-resident feature table.  Replaces what feeds the step in the reference: TennisSet.__getitem__
 * opening one .npy per window step (dataset.py:190-213), the loader stacking them to (B, T, F) and the per-batch copy to the
 * device in front of ag.record / backward / trainer.step (train.py:410-424).  The table is uploaded once; a step names its
 * window rows, and the two kernels that read the (B*T, F) window matrix (the i2h projection and dW_ih = dGI^T X) gather them
 * while they stage the operand, in the arithmetic order of the materialised step: the results are bit-identical to
 * tn_head_forward_backward on the gathered matrix.
 * set_features: feats (rows, F) fp32 DEVICE of row stride ld >= F floats; BORROWED, not copied - it must stay alive and
 *   unchanged while rows calls use it; a later set_features replaces it.
 * forward_backward_rows: row_idx (batch * steps) int32 DEVICE in order b * steps + t; an index is clamped to [0, rows - 1]
 *   inside the kernels, so no content of the array reads outside the table.  Everything else as tn_head_forward_backward.
 * forward_rows: the forward half only, logits (batch, classes) fp32 DEVICE; gradients, momentum and parameters untouched.
 * A rows call before set_features, null arguments and batch or steps over the handle's maxima are TN_ERR_INVALID.  No call
 * allocates. */
int tn_head_set_features(tn_head *h, const float *feats, int rows, int ld);
int tn_head_forward_backward_rows(tn_head *h, const int32_t *row_idx, const int32_t *labels, int batch, int steps, float *loss,
                                  float *logits);
int tn_head_forward_rows(tn_head *h, const int32_t *row_idx, int batch, int steps, float *logits);
int tn_head_buffers(tn_head *h, float **params_dev, float **grads_dev, int64_t *numel);
int tn_head_sgd_step(tn_head *h, float lr, float momentum, float wd, float rescale_grad);
int tn_head_read_param(tn_head *h, const char *name, int gradient, float *out_host, int64_t capacity, int64_t *numel);
int tn_head_destroy(tn_head *h);

/* ---- fine-tuning step of the frame classifier (second half) ------ */
/* FrameModel(DenseNet-121 .features, Dense(classes)) trained end to end as reference train.py does when the backbone is
 * not frozen: BatchNorm in training mode (batch statistics; running statistics updated with momentum 0.9),
 * SoftmaxCrossEntropyLoss per sample (train.py:324), backward of the summed losses (:419-421), SGD with momentum and
 * weight decay, rescale_grad = 1/batch_size (:298-299,424).  fp32.  Parameters by their Gluon names (as
 * tn_densenet121_create + the Dense).  x (batch, H, W, 3) fp32 normalised NHWC frames and labels (batch,) int32 are
 * DEVICE buffers; batch, height and width must equal the handle's (the frame buffer is read as batch x height x width x 3).  read_param returns Gluon-ordered weights / gradients, running
 * statistics, or "<bn>_batch_mean" / "<bn>_batch_var" of the last step. */
typedef struct tn_finetune tn_finetune;
int tn_finetune_create(tn_ctx *ctx, const tn_param *params, int n_params, const char *backbone_prefix,
                       const char *dense_prefix, int height, int width, int classes, int batch, tn_finetune **out);
int tn_finetune_forward_backward(tn_finetune *f, const float *x, const int32_t *labels, int batch, int height, int width, float *loss,
                                 float *logits);
int tn_finetune_buffers(tn_finetune *f, float **params_dev, float **grads_dev, int64_t *numel);
int tn_finetune_sgd_step(tn_finetune *f, float lr, float momentum, float wd, float rescale_grad);
int tn_finetune_read_param(tn_finetune *f, const char *name, int gradient, float *out_host, int64_t capacity,
                           int64_t *numel);
int tn_finetune_destroy(tn_finetune *f);
/* The matrix pipe of the backbone's GEMMs (the convolutions of reference train.py:410-424's record / backward, as GEMMs: the stem, the
 * 58 x 2 dense-layer convolutions and the 3 transitions forward, their weight and input gradients backward).  TN_MATMUL_F32, the
 * default: the exact-f32 matrix instruction.  TN_MATMUL_FP32X3: fp32 operands, accumulators and results with every operand value
 * split into three bf16 terms and the six largest cross products on the bf16 matrix pipe (csrc/gemm_fp32x3.hip) - the same
 * float64 bars, a kernel error below 5e-7 of sum |a||b|; a value beyond bf16's finite range (3.39e38) splits to NaN.  The mode
 * may change between steps; an unknown value is an error.  Not switched: the classifier, the recurrent head, the captioner.
 * matmul_stats: backbone GEMM launches per mode since creation (a trainable step: 120 forward + 239 backward); either may be NULL. */
#define TN_MATMUL_F32 0
#define TN_MATMUL_FP32X3 1
int tn_finetune_set_matmul(tn_finetune *f, int mode);
int tn_finetune_matmul_stats(tn_finetune *f, int64_t *f32_launches, int64_t *fp32x3_launches);

/* ---- end-to-end CNN-RNN training step ---------------------------- */
/* CNNRNN(FrameModel(DenseNet-121 .features)) over TimeDistributed frames, trained as reference train.py:197-236 does with
 * --window > 1 --temp_pool gru|lstm and no --feats_model: DenseNet-121 .features (BatchNorm in training mode over all
 * batch x steps frames, which TimeDistributed merges into one batch, utils/layers.py:38-46) -> features (batch*steps, 1024) in frame
 * order b*steps + t -> bi-GRU / bi-LSTM -> max over T -> Dense(classes) (definitions.py:75-110) -> SoftmaxCrossEntropyLoss per
 * sample (train.py:324) -> backward of the summed losses (:419-421) through the head and, unless the backbone is frozen
 * (--freeze_backbone, :231-233), through the backbone -> SGD with momentum and weight decay (:298-299,424).  fp32.
 * Frozen: no backbone backward and no backbone update; its BatchNorms still normalise with batch statistics and still update
 * their running statistics (MXNet under ag.record() with grad_req 'null').  The hidden size is read from the parameters.
 * create: kind as tn_head_create; prefixes of the backbone (e.g. "densenet0_"), the recurrent layer ("cnnrnn0_gru0_") and the
 * Dense ("cnnrnn0_dense0_"); square frames of a side divisible by 32.  When batch * steps frames do not fit the device, create
 * returns TN_ERR_NOMEM and its message gives the frames that would.
 * forward_backward: x (batch, steps, height, width, 3) fp32 normalised NHWC frames and labels (batch,) int32, DEVICE; batch,
 * steps, height and width must equal the handle's.  loss (batch,) / logits (batch, classes): optional device outputs.
 * buffers: the flat parameter / gradient arrays of the backbone (as tn_finetune_buffers) and of the head (as tn_head_buffers),
 * e.g. to all-reduce them over ranks before sgd_step; any output pointer may be NULL.
 * read_param: the Gluon names of both parts, the backbone's running statistics and its "<bn>_batch_mean" / "<bn>_batch_var". */
typedef struct tn_cnnrnn_trainer tn_cnnrnn_trainer;
int tn_cnnrnn_trainer_create(tn_ctx *ctx, tn_rnn_kind kind, const tn_param *params, int n_params, const char *backbone_prefix,
                             const char *rnn_prefix, const char *dense_prefix, int height, int width, int classes, int batch,
                             int steps, int freeze_backbone, tn_cnnrnn_trainer **out);
int tn_cnnrnn_trainer_forward_backward(tn_cnnrnn_trainer *t, const float *x, const int32_t *labels, int batch, int steps,
                                       int height, int width, float *loss, float *logits);
int tn_cnnrnn_trainer_buffers(tn_cnnrnn_trainer *t, float **backbone_params, float **backbone_grads, int64_t *backbone_numel,
                              float **head_params, float **head_grads, int64_t *head_numel);
int tn_cnnrnn_trainer_sgd_step(tn_cnnrnn_trainer *t, float lr, float momentum, float wd, float rescale_grad);
int tn_cnnrnn_trainer_read_param(tn_cnnrnn_trainer *t, const char *name, int gradient, float *out_host, int64_t capacity,
                                 int64_t *numel);
int tn_cnnrnn_trainer_destroy(tn_cnnrnn_trainer *t);
/* tn_finetune_set_matmul / _matmul_stats of the step's backbone (reference train.py:410-424); a frozen step counts its 120 forward launches */
int tn_cnnrnn_trainer_set_matmul(tn_cnnrnn_trainer *t, int mode);
int tn_cnnrnn_trainer_matmul_stats(tn_cnnrnn_trainer *t, int64_t *f32_launches, int64_t *fp32x3_launches);

/* ---- captioner training step ---------------------------------- */
/* One step of reference train_gnmt.py::train (:328-337) for GRU or LSTM cells (--cell_type), num_layers = 2,
 * num_bi_layers = 1:
 *   out, _ = model(src, tgt[:, :-1], src_valid_length, tgt_valid_length - 1)        teacher-forced NMTModel.forward
 *   loss = MaskedSoftmaxCELoss(out, tgt[:, 1:], tgt_valid_length - 1).mean()
 *          * (tgt.shape[1] - 1) / (tgt_valid_length - 1).mean()                      = summed NLL / number of valid tokens
 *   loss.backward(); gluon.Trainer(params, 'adam', {'learning_rate': lr}).step(1)   MXNet Adam [EXT]
 * Parameters use the names of tn_gnmt_create.  forward_backward takes DEVICE buffers: src (batch, steps, input_size)
 * fp32, tgt (batch, ld) int32 of which tgt_len columns are used, valid lengths (batch,) int32 (tgt_valid_len counts BOS
 * and EOS, as the reference's data loader gives it); loss is one device float, logits_out (batch, tgt_len-1, vocab)
 * optional.  The gradient of the loss w.r.t. every parameter is left in the flat gradient buffer
 * (tn_gnmt_trainer_buffers; all-reduce it over ranks for data parallelism) for tn_gnmt_trainer_adam_step. */
typedef struct tn_gnmt_trainer tn_gnmt_trainer;
int tn_gnmt_trainer_create(tn_ctx *ctx, const tn_param *params, int n_params, const char *prefix, tn_rnn_kind cell_kind,
                           int input_size, int hidden, int embed, int vocab, int max_batch, int max_src_len,
                           int max_tgt_len, tn_gnmt_trainer **out);
/* Any layer count the inference handle serves (tn_gnmt_create_ex): num_layers >= 2, 0 <= num_bi_layers < num_layers, flags =
 * TN_GNMT_USE_RESIDUAL or 0 - the arguments the reference passes into the model it trains (train_gnmt.py:58-61,223-227;
 * models/captioning/gnmt.py:71-111,153-157,393-396).  Parameter names: enc_rnn{i}_l_ / _r_ (bidirectional layers), enc_rnn{i}_,
 * dec_rnn{j}_.  tn_gnmt_trainer_create = (2, 1, 0), the reference's flag defaults.  hidden % 4 == 0 and gates*hidden <= 2048
 * (--num_hidden up to 680 with GRU cells, 512 with LSTM cells), the encoder's bound as in tn_birnn_create. */
int tn_gnmt_trainer_create_ex(tn_ctx *ctx, const tn_param *params, int n_params, const char *prefix, tn_rnn_kind cell_kind,
                              int input_size, int hidden, int embed, int vocab, int num_layers, int num_bi_layers, int flags,
                              int max_batch, int max_src_len, int max_tgt_len, tn_gnmt_trainer **out);
int tn_gnmt_trainer_forward_backward(tn_gnmt_trainer *t, const float *src, const int32_t *src_valid_len,
                                     const int32_t *tgt, int ld, const int32_t *tgt_valid_len, int batch, int steps,
                                     int tgt_len, float *loss, float *logits_out);
/* The same step from a device-resident feature table.  Replaces what feeds the step in the reference's feature mode: TennisSet.
 * __getitem__ opening one .npy per frame of every point of the batch (dataset.py:161-178), the batchify function stacking them into a
 * zero-padded (B, T, F) array and the per-batch copy to the device in front of the step (train_gnmt.py:318-337).  The table (n_rows,
 * input_size) fp32 DEVICE of row stride ld >= input_size floats is uploaded once by the caller and only read here: the call keeps no
 * pointer to it.  row_idx (batch * steps) int32 DEVICE in order b * steps + t names each step's row; a NEGATIVE index is a pad step
 * (behind a clip shorter than the batch's longest) and stands for a row of zeros, an index >= n_rows is clamped to n_rows - 1, so no
 * content of the array reads outside the table.  The two kernels that read src - encoder layer 0's i2h product and dW_ih = dGI^T src -
 * gather the rows while they stage them, in the arithmetic order of the materialised step: loss, logits and gradients are
 * bit-identical to tn_gnmt_trainer_forward_backward on the zero-padded batch.  Everything else as that call; n_rows < 1, ld <
 * input_size and null arguments are TN_ERR_INVALID.  No call allocates. */
int tn_gnmt_trainer_forward_backward_rows(tn_gnmt_trainer *t, const float *table, int n_rows, int ld, const int32_t *row_idx,
                                          const int32_t *src_valid_len, const int32_t *tgt, int ld_tgt, const int32_t *tgt_valid_len,
                                          int batch, int steps, int tgt_len, float *loss, float *logits_out);
int tn_gnmt_trainer_buffers(tn_gnmt_trainer *t, float **params_dev, float **grads_dev, int64_t *numel);
/* --dropout of train_gnmt.py (gnmt.py:152,395: after each encoder layer and on the top decoder cell's output), inverted
 * dropout from a counter-based generator; 0 until set.  tn_gnmt_trainer_dropout_masks: the last step's masks (test hook). */
int tn_gnmt_trainer_set_dropout(tn_gnmt_trainer *t, float p, uint64_t seed);
int tn_gnmt_trainer_dropout_masks(tn_gnmt_trainer *t, float **m_enc0, float **m_enc1, float **m_dec);
/* one mask of the last step (test hook): which = encoder layer 0 .. num_layers - 1 -> (B*T, dirs*H); num_layers + j -> decoder layer
 * j >= 1, (L*B, H) step-major */
int tn_gnmt_trainer_dropout_mask(tn_gnmt_trainer *t, int which, float **mask);
int tn_gnmt_trainer_adam_step(tn_gnmt_trainer *t, float lr, float beta1, float beta2, float epsilon);
int tn_gnmt_trainer_read_param(tn_gnmt_trainer *t, const char *name, int gradient, float *out_host, int64_t capacity,
                               int64_t *numel);
int tn_gnmt_trainer_destroy(tn_gnmt_trainer *t);

/* ---- end-to-end frame-mode captioner training step --------------- */
/* train_gnmt.py without --feats_model (:148-203): the source embedding is TimeDistributed(FrameModel(DenseNet-121 .features)
 * .backbone) inside the NMTModel, so one step runs the backbone in training mode over all batch x steps frames of the padded
 * clips (utils/layers.py:38-46), the captioner step above on its features (rows b*steps + t), and - unless the backbone is frozen
 * (--freeze_backbone, :164-166) - carries d loss / d src back through the backbone.  fp32.
 * create (:149-186, 223-229): the arguments of tn_gnmt_trainer_create_ex without input_size, which is the backbone's feature
 * width (parameters whose first encoder layer has another width are refused), plus the backbone's prefix ("densenet0_"), the
 * side of the square frames (divisible by 32), max_frames >= the largest batch * steps of a call, and freeze_backbone.  When
 * max_frames do not fit the device, create returns TN_ERR_NOMEM and its message gives the frames that would.
 * forward_backward (:328-334): frames (batch, steps, side, side, 3) fp32 normalised NHWC, DEVICE; the other arguments as
 * tn_gnmt_trainer_forward_backward.  Any batch <= max_batch, steps <= max_src_len with batch * steps <= max_frames.  The frames
 * are read once into the handle's staging buffer, the slots t >= src_valid_len[b] as zeros - what Pad() puts there
 * (utils/captioning.py:33) - whatever the caller left in them (they are not read); the padded slots go through the backbone with
 * the others and count in its batch statistics, as in the reference.  The caller's buffer is not written.
 * Frozen: no backbone backward and no backbone update; its BatchNorms still normalise with batch statistics and still update
 * their running statistics (as tn_cnnrnn_trainer_*).
 * buffers: the flat parameter / gradient arrays of the backbone (as tn_finetune_buffers) and of the captioner (as
 * tn_gnmt_trainer_buffers), e.g. to all-reduce them over ranks before adam_step; any output pointer may be NULL.
 * adam_step (:310,337): MXNet Adam over both parts, one update count; the running statistics are not parameters.
 * read_param: the names of both parts, the backbone's running statistics and its "<bn>_batch_mean" / "<bn>_batch_var". */
typedef struct tn_gnmt_frames_trainer tn_gnmt_frames_trainer;
int tn_gnmt_frames_trainer_create(tn_ctx *ctx, const tn_param *params, int n_params, const char *backbone_prefix, const char *prefix,
                                  tn_rnn_kind cell_kind, int hidden, int embed, int vocab, int num_layers, int num_bi_layers, int flags,
                                  int side, int max_batch, int max_src_len, int max_tgt_len, int max_frames, int freeze_backbone,
                                  tn_gnmt_frames_trainer **out);
int tn_gnmt_frames_trainer_forward_backward(tn_gnmt_frames_trainer *t, const float *frames, const int32_t *src_valid_len,
                                            const int32_t *tgt, int ld, const int32_t *tgt_valid_len, int batch, int steps,
                                            int tgt_len, float *loss, float *logits_out);
int tn_gnmt_frames_trainer_buffers(tn_gnmt_frames_trainer *t, float **backbone_params, float **backbone_grads,
                                   int64_t *backbone_numel, float **params_dev, float **grads_dev, int64_t *numel);
int tn_gnmt_frames_trainer_set_dropout(tn_gnmt_frames_trainer *t, float p, uint64_t seed);
int tn_gnmt_frames_trainer_adam_step(tn_gnmt_frames_trainer *t, float lr, float beta1, float beta2, float epsilon);
int tn_gnmt_frames_trainer_read_param(tn_gnmt_frames_trainer *t, const char *name, int gradient, float *out_host,
                                      int64_t capacity, int64_t *numel);
int tn_gnmt_frames_trainer_destroy(tn_gnmt_frames_trainer *t);
/* tn_finetune_set_matmul / _matmul_stats of the step's backbone (reference train_gnmt.py:148-203); the captioner's own GEMMs stay f32 */
int tn_gnmt_frames_trainer_set_matmul(tn_gnmt_frames_trainer *t, int mode);
int tn_gnmt_frames_trainer_matmul_stats(tn_gnmt_frames_trainer *t, int64_t *f32_launches, int64_t *fp32x3_launches);

/* ---- global-norm gradient clipping of the five training steps (opt-in) ------------------
 * gluon.utils.clip_global_norm(grads, clip) [EXT], the call the gluonnlp script behind reference train_gnmt.py makes between
 * loss.backward() and trainer.step(1).  The reference defines the flag (train_gnmt.py:97-98, --clip) and never applies it; so
 * clipping is OFF after every create, and a handle that never calls set_clip runs the steps it always ran, bit for bit.
 *   norm  = sqrt(sum over every TRAINABLE gradient element of (r g)^2)      r = rescale_grad of the sgd_step, 1 for adam_step
 *   scale = min(1, max_norm / (norm + 1e-8))
 *   the update runs on scale g in place of g  (SGD: mom = momentum mom - lr (r scale g + wd w);  Adam: g' = scale g)
 * The SGD norm is taken over r g, the gradient the optimizer sees, so a threshold keeps its meaning when the batch size changes.
 * The gradient buffers are not modified (*_buffers / read_param(gradient = 1) still show the unclipped gradient): the scale is
 * applied inside the update kernel.  Below the threshold scale is exactly 1 and the step leaves the bits of an unclipped one.  A
 * non-finite norm propagates as the formula says (MXNet warns and goes on).  A frozen backbone adds nothing to the norm; the
 * two-part handles take ONE norm over backbone + head / captioner and give both parts the one scale.  The sum is a two-stage
 * reduction in a fixed order (no atomics): equal gradients give equal bits on every rank.  No host synchronisation in a step.
 * set_clip: max_norm 0 switches clipping off; negative or non-finite is TN_ERR_INVALID.
 * clip_stats: the last step's norm and scale and the steps with scale < 1 since create (any pointer may be NULL); synchronises
 * the handle's stream, so call it per epoch or log point, not per step; an error while clipping is off or before a clipped step. */
int tn_head_set_clip(tn_head *h, float max_norm);
int tn_head_clip_stats(tn_head *h, float *norm, float *scale, int64_t *clipped_steps);
int tn_finetune_set_clip(tn_finetune *f, float max_norm);
int tn_finetune_clip_stats(tn_finetune *f, float *norm, float *scale, int64_t *clipped_steps);
int tn_cnnrnn_trainer_set_clip(tn_cnnrnn_trainer *t, float max_norm);
int tn_cnnrnn_trainer_clip_stats(tn_cnnrnn_trainer *t, float *norm, float *scale, int64_t *clipped_steps);
int tn_gnmt_trainer_set_clip(tn_gnmt_trainer *t, float max_norm);
int tn_gnmt_trainer_clip_stats(tn_gnmt_trainer *t, float *norm, float *scale, int64_t *clipped_steps);
int tn_gnmt_frames_trainer_set_clip(tn_gnmt_frames_trainer *t, float max_norm);
int tn_gnmt_frames_trainer_clip_stats(tn_gnmt_frames_trainer *t, float *norm, float *scale, int64_t *clipped_steps);

/* ---- device PRF1 confusion histogram -------------------------------------- */
/* Replaces the argmax + per-sample python loop of PRF1.update (reference
 * metrics/vision.py:41-49).  logits (rows,classes) fp32, labels (rows,) int32;
 * adds into mat (classes*classes) int64, row = label, col = argmax (first max).
 * Rows whose label lies outside 0..classes-1 are dropped, and mat.sum() grows by
 * the number of in-range labels. */
int tn_prf1_update(tn_ctx *ctx, const float *logits, const int32_t *labels, int rows, int classes,
                   int64_t *mat);

/* ---- events from per-frame logits (csrc/event_runs.hip; docs/kernels.md "Event decoding") ----
 * Turns the (N, C) fp32 DEVICE logits of an evaluation into events "class c, positions first..last, score".  Has no counterpart in
 * the reference, whose per-frame results go into visualise_events on the host.
 *   inputs   rows (M,) int32: position m of the time-ordered list reads logits[clamp(rows[m], 0, N-1)], unconditionally (any
 *            selection or permutation: a split's samples are not stored in time order); start (M,) int32: non-zero where position m
 *            begins a new video, position 0 always does; width odd in [1, 63]; C in [1, 64].
 *   p        p[m] = softmax of that row: maximum subtracted, accurate expf, the sum in ascending c, one division per value.
 *   score    score[m, c] = (sum_{j = lo..hi} p[j, c]) / (hi - lo + 1), j ascending, lo = max(m - h, first position of m's video),
 *            hi = min(m + h, last position of m's video), h = (width - 1) / 2: the direct sum of at most 63 terms, no sliding sum, so
 *            that no score depends on where a tile begins.  A window of one position is p's bits, with no division.
 *   label    label[m] = the first arg-max of score[m] (a tie goes to the smallest class), conf[m] = score[m, label[m]].
 *   events   a maximal stretch of positions of one video with one label.  Per event first, last (positions, inclusive), cls,
 *            peak = the maximum conf and score = the mean conf, summed in an order that depends on the event's own positions only
 *            (lane l of a wave takes first + l, first + l + 64, ... ascending, then a six-level xor tree 32, 16, ..., 1; one
 *            division by the length).  Events come out ordered by first; *count = K <= M.
 * So a video decoded alone gives the bits of its events inside a whole-corpus call, nothing depends on grid or tile size, and there
 * are no atomics on floats.  A run of the "other" class is an event too; smoothing moves boundaries by up to h positions.
 * create: workspace for up to max_positions positions (9 bytes each and 8 per 128) - run allocates nothing.
 * run: label_out (M,) int32 and conf_out (M,) fp32 may be NULL; ev_first, ev_last, ev_cls (int32) and ev_score, ev_peak (fp32) hold
 * M entries each, of which the first K are written; count is ONE DEVICE int32.  stream: a hipStream_t, NULL = the context's
 * stream; the call is asynchronous on it.  All pointers DEVICE.  TN_ERR_INVALID with the argument named in tn_last_error for: a
 * null pointer (label_out / conf_out excepted), N < 1, C outside [1, 64] or past max_classes, an even width, width outside
 * [1, 63], M < 1, M > max_positions. */
typedef struct tn_event_decoder tn_event_decoder;
int tn_event_decoder_create(tn_ctx *ctx, int max_positions, int max_classes, tn_event_decoder **out);
int tn_event_decoder_run(tn_event_decoder *d, const float *logits, int N, int C, const int32_t *rows, const int32_t *start, int M,
                         int width, int32_t *label_out, float *conf_out, int32_t *ev_first, int32_t *ev_last, int32_t *ev_cls,
                         float *ev_score, float *ev_peak, int32_t *count, void *stream);
int tn_event_decoder_destroy(tn_event_decoder *d);

/* The same events from the label path that maximises the sum of the per-position scores minus switch_cost for every change of label
 * inside a video (a Potts model, decoded with Viterbi; docs/kernels.md "Event decoding with a switch cost").  Arguments as
 * tn_event_decoder_run, with float switch_cost (finite, >= 0, in logit = natural-log units) in place of the window width.
 *   e        e[m, c] = q[c] - max_c q[c], q = logits[clamp(rows[m], 0, N-1)], fp32.  The log-sum-exp is not subtracted: it is the
 *            same for every class of a position and cannot change the path.
 *   forward  per video, positions t = 0 .. T-1 in order, fp32:  v_0 = e_0;  stay_t[c] = (v_{t-1}[c] >= -switch_cost);
 *            u_t[c] = e_t[c] + max(v_{t-1}[c], -switch_cost);  v_t[c] = u_t[c] - max_c u_t[c];  a_t = the first arg-max of v_t.
 *            The best predecessor scores 0 after the normalisation, so switching in is worth exactly -switch_cost, and every value
 *            stays within [-(switch_cost + max|e|), 0] however long the video is.  A tie between staying and switching stays.
 *   back     label[T-1] = a_{T-1};  label[t-1] = stay_t[label[t]] ? label[t] : a_{t-1}.
 *   conf     conf[m] = softmax(q)[label[m]]: maximum subtracted, accurate expf, the sum in ascending c, one division - the bits
 *            tn_event_decoder_run gives at width 1 for that class.
 *   events   from label, conf and start exactly as tn_event_decoder_run's.
 * The order is sequential by definition (fp32 max-plus does not round associatively): one workgroup walks one video, no workgroup
 * waits on another, there are no atomics on floats, and no value depends on the grid or on the tile, so a video decoded alone gives
 * the bits it gives inside a whole-corpus call.  switch_cost = 0 gives the first arg-max of every row that has no tied maximum.
 * The first call allocates the path workspace inside the handle (13 bytes per position of max_positions; TN_ERR_NOMEM with the size
 * in tn_last_error if that fails); later calls allocate nothing, and tn_event_decoder_run never touches it.  TN_ERR_INVALID as
 * tn_event_decoder_run, and for a switch_cost that is negative, NaN or infinite. */
int tn_event_decoder_run_switch(tn_event_decoder *d, const float *logits, int N, int C, const int32_t *rows, const int32_t *start,
                                int M, float switch_cost, int32_t *label_out, float *conf_out, int32_t *ev_first, int32_t *ev_last,
                                int32_t *ev_cls, float *ev_score, float *ev_peak, int32_t *count, void *stream);

/* The same events from the label path under a class-transition matrix (an HMM on top of the frame classifier, decoded with Viterbi;
 * docs/kernels.md "Event decoding with a transition matrix").  Arguments as tn_event_decoder_run_switch, with the matrix in place of
 * the cost: transitions is a HOST pointer to (C, C) floats, row-major, transitions[from * C + to] = T[from][to] the score added when a
 * position labelled `from` is followed inside the same video by one labelled `to`.  Every entry is finite and <= 0, or -inf (the
 * transition is forbidden); the diagonal is finite, so staying is always possible and every value below stays finite.  The matrix
 * is checked on the host, then copied into the handle with hipMemcpyAsync on the call's stream (keep pinned memory unchanged until
 * the stream has passed the copy).
 *   e        as above.  The path maximises  sum_m e[m, label[m]] + sum_{m not its video's first} T[label[m-1]][label[m]].
 *   forward  per video, positions in order, fp32, every sum rounded:  v_0 = e_0;  w_t[c] = max_p (v_{t-1}[p] + T[p][c]);
 *            b_t[c] = c if v_{t-1}[c] + T[c][c] attains w_t[c] (staying wins a tie), else the smallest p that attains it;
 *            u_t[c] = e_t[c] + w_t[c];  v_t[c] = u_t[c] - max_c u_t[c];  a_t = the first arg-max of v_t.
 *   back     label[T-1] = a_{T-1};  label[t-1] = b_t[label[t]].
 *   conf, events   exactly as tn_event_decoder_run_switch's.
 * With T = -cost (1 - I) every u and v is the switch-cost recurrence's bit for bit (the best predecessor has v = 0 and the rounded
 * sums v[p] - cost are monotone in v[p]).  Sequential by definition, one workgroup per video, no workgroup waits on another, no
 * atomics on floats, nothing depends on grid or tile: a video decoded alone gives the bits of the whole-corpus call.  Every stored
 * index lies in [0, C) whatever the floats are; with a NaN among the logits the labels are unspecified but in range.
 * The first call allocates the back-pointer workspace inside the handle: (pitch + 5) bytes per position of max_positions (rounded up
 * to a multiple of 4), pitch = 16 for max_classes <= 16 and 64 above, plus 4 max_classes^2 + 4 bytes; TN_ERR_NOMEM with the size in
 * tn_last_error if that fails.  Later calls allocate nothing, and the other two run entries never touch it.  TN_ERR_INVALID as
 * tn_event_decoder_run_switch, for a null transitions, and - naming the first offending [from][to] - for an entry that is NaN, an
 * entry that is positive (+inf included), and a diagonal entry that is not finite. */
int tn_event_decoder_run_transitions(tn_event_decoder *d, const float *logits, int N, int C, const int32_t *rows, const int32_t *start,
                                     int M, const float *transitions, int32_t *label_out, float *conf_out, int32_t *ev_first,
                                     int32_t *ev_last, int32_t *ev_cls, float *ev_score, float *ev_peak, int32_t *count, void *stream);

/* The events of tn_event_decoder_run_transitions, scored with the HMM's own posteriors (forward-backward; docs/kernels.md "Event scores
 * from posteriors").  Arguments as tn_event_decoder_run_transitions, plus float *posterior: DEVICE memory for (M, C) floats, row-major,
 * may be NULL.
 *   label    the Viterbi path under the matrix: the bits of tn_event_decoder_run_transitions.
 *   gamma    gamma_t[c] = P(label_t = c | every position of the video) under the HMM with emissions e and transitions T, per video in
 *            the log domain, fp32, LSE(x) = mx + ln sum_i exp(x_i - mx) with mx = max x, the sum in ascending i, a -inf term adding 0:
 *            forward   a_0 = e_0;  a_t[c] = e_t[c] + LSE_p(ah_{t-1}[p] + T[p][c]);  ah_t = a_t - max_c a_t;
 *            backward  b_{L-1} = 0;  b_t[p] = LSE_c(T[p][c] + (e_{t+1}[c] + bh_{t+1}[c]));  bh_t = b_t - max_p b_t;
 *            gamma_t = softmax_c(ah_t + bh_t): maximum subtracted, expf, the sum in ascending c, one division per value.
 *            The finite diagonal keeps every b_t[p] and at least one a_t[c] finite, so no value is NaN however far the logits
 *            lie apart and whatever the matrix forbids; a class that cannot be reached has gamma = 0.
 *   posterior  gamma, if not NULL.
 *   conf     conf[m] = gamma_m[label[m]], the bits stored in posterior.  score and peak of an event are the mean and maximum of that.
 *   events   from label, conf and start exactly as tn_event_decoder_run's.
 * Each direction of each video is one workgroup's sequential walk, both directions of all videos in one launch; no workgroup waits
 * on another, there are no atomics on floats and nothing depends on grid or tile: a video decoded alone gives the bits of the
 * whole-corpus call.  The first call allocates the posterior workspace inside the handle, 2 * max_positions * pitch * 4 bytes for ah
 * and bh, pitch = 16 for max_classes <= 16 and 64 above (and the back-pointer workspace, if no tn_event_decoder_run_transitions has);
 * TN_ERR_NOMEM with the size in tn_last_error if that fails.  Later calls allocate nothing, and the other run entries never touch it.
 * TN_ERR_INVALID exactly as tn_event_decoder_run_transitions. */
int tn_event_decoder_run_posteriors(tn_event_decoder *d, const float *logits, int N, int C, const int32_t *rows, const int32_t *start,
                                    int M, const float *transitions, int32_t *label_out, float *conf_out, float *posterior,
                                    int32_t *ev_first, int32_t *ev_last, int32_t *ev_cls, float *ev_score, float *ev_peak, int32_t *count,
                                    void *stream);

/* ---- multi-GPU exchange: RCCL over xGMI, one process per GPU (csrc/comm.hip) ------------
 * The path's one exchange step (BASELINE config C4).  The reference splits every DataLoader batch over its ctx list and
 * exchanges the per-frame feature rows through the file system: evaluate.py:278-281,308-321 writes
 * <root>/features/<model_id>/<video>/<frame>.npy, dataset.py:202-204 np.load()s them for the temporal / caption stage.
 * Here every rank keeps its shard of feature rows in HBM and one all-gather puts the whole (N, F) matrix on every rank.
 * Also: the sum / mean of the three trainers' flat gradient buffers (train.py:410-424 `trainer.step` over a ctx list =
 * kvstore 'device' all-reduce) and of the PRF1 confusion counts.
 *
 * Rank 0 calls tn_comm_unique_id and hands the 128 bytes to the other ranks by any out-of-band channel (a file, a TCP
 * store, MPI); every rank then calls tn_comm_create with its own context (one process per GPU, the context's device).
 * All collectives are asynchronous and ordered on the context's stream like every other entry point; librccl is opened
 * at run time (a process that already holds one - PyTorch's - shares it), a world of 1 needs none (TN_COMM_FORCE_RCCL
 * makes a single rank go through RCCL all the same: the self-test of 1-GPU boxes). */
#define TN_UNIQUE_ID_BYTES 128
#define TN_COMM_FORCE_RCCL 1
typedef struct tn_comm tn_comm;
int tn_comm_unique_id(void *id_out /* TN_UNIQUE_ID_BYTES */);
int tn_comm_create(tn_ctx *ctx, int rank, int world, const void *unique_id /* NULL for world 1 */, int flags,
                   tn_comm **out);
/* What the communicator itself reports (with RCCL behind the handle: ncclCommUserRank / ncclCommCount / ncclCommCuDevice, so a
 * record of an N-GPU run shows that RCCL saw N ranks - the reference's counterpart is len(ctx) at evaluate.py:84-85); -1 when RCCL
 * refuses the query.  tn_comm_uses_rccl: 0 for the world-1 short cut that needs no RCCL. */
int tn_comm_rank(const tn_comm *c);
int tn_comm_world(const tn_comm *c);
int tn_comm_device(const tn_comm *c);
int tn_comm_uses_rccl(const tn_comm *c);
/* out (world*rows, F) = rank-major concatenation of every rank's shard (rows, F); equal `rows` on every rank (pad the last
 * round, sharding.local_rows); shard may alias its own slot of out. */
int tn_allgather_features(tn_comm *c, const float *shard, int rows, int F, float *out);
/* in place; average != 0 divides by the world size (Trainer.step's rescale) */
int tn_allreduce_f32(tn_comm *c, float *buf, size_t n, int average);
int tn_allreduce_i64(tn_comm *c, int64_t *buf, size_t n);
int tn_comm_destroy(tn_comm *c);

/* ---- GNMT captioner: encoder + attention decoder + beam search -------------- */
/* Replaces get_gnmt_encoder_decoder / NMTModel / BeamSearchTranslator as assembled at
 * reference train_gnmt.py:223-252 and driven by evaluate() (train_gnmt.py:264-302):
 *   tn_gnmt_encode      = model.encode -> GNMTEncoder.forward (models/captioning/gnmt.py:136-160)
 *                         + decoder.init_state_from_encoder (gnmt.py:224-252)
 *   tn_gnmt_beam_search = BeamSearchTranslator.translate (utils/translation.py:55-82): the whole
 *                         decode_step / log_softmax / BeamSearchSampler loop on the device.
 * params: "<prefix>enc_rnn{i}_{l,r}_*" for the num_bi_layers bidirectional encoder layers, "<prefix>enc_rnn{i}_*" for
 * the uni-directional ones, "<prefix>dec_rnn{i}_*" ({i2h,h2h}_{weight,bias}; i < num_layers),
 * "<prefix>dec_attention_key_weight" (H,H), "<prefix>tgt_proj_{weight,bias}", "<prefix>tgt_embed_weight" (V,E).
 * cell_type gru | lstm, 2 <= num_layers <= 8, 0 <= num_bi_layers < num_layers (gnmt.py:78-80; with every layer
 * bidirectional the memory is 2H wide, which gluonnlp's Luong attention with units = H refuses), scaled_luong attention,
 * dropout off (inference); tn_gnmt_create_ex(flags = TN_GNMT_USE_RESIDUAL): use_residual (gnmt.py:155-157,394-395).
 * src (B,T,F) fp32 features, valid_len (B,) int32; samples (B,beam,max_length+2) int32 padded
 * with -1 (leading BOS), scores (B,beam) descending, valid_length (B,beam) int32;
 * *length_host = number of meaningful columns of `samples` (the width the reference returns). */
int tn_gnmt_create(tn_ctx *ctx, const tn_param *params, int n_params, const char *prefix, int cell_kind,
                   int input_size, int hidden, int embed, int vocab, int num_layers, int num_bi_layers,
                   int max_batch, int max_src_len, int beam, int max_length, tn_gnmt **out);
#define TN_GNMT_USE_RESIDUAL 1
int tn_gnmt_create_ex(tn_ctx *ctx, const tn_param *params, int n_params, const char *prefix, int cell_kind,
                      int input_size, int hidden, int embed, int vocab, int num_layers, int num_bi_layers,
                      int max_batch, int max_src_len, int beam, int max_length, int flags, tn_gnmt **out);
int tn_gnmt_encode(tn_gnmt *g, const float *src, const int32_t *valid_len, int batch, int steps, float *mem_out);
/* tn_gnmt_encode from a device-resident feature table: what evaluate() (train_gnmt.py:264-302) and evaluate_gnmt.py feed model.encode
 * with, minus the loader - one .npy per frame of every point (dataset.py:161-178), the padded (B, T, F) batch and its copy, for every
 * batch of every validation and test pass.  table, n_rows, ld and row_idx (batch * steps, negative = a pad step = zeros, >= n_rows
 * clamped) as in tn_gnmt_trainer_forward_backward_rows; encoder layer 0's i2h product gathers the rows, and mem, the states and the
 * key projection are bit-identical to tn_gnmt_encode on the zero-padded batch.  tn_gnmt_decode_seq / tn_gnmt_beam_search follow it
 * as they follow tn_gnmt_encode. */
int tn_gnmt_encode_rows(tn_gnmt *g, const float *table, int n_rows, int ld, const int32_t *row_idx, const int32_t *valid_len, int batch,
                        int steps, float *mem_out);
int tn_gnmt_beam_search(tn_gnmt *g, int bos, int eos, float alpha, float K, int max_length, int32_t *samples,
                        float *scores, int32_t *valid_length, int *length_host);
/* Teacher forcing: model(src, tgt[:, :-1], ...) of evaluate() (train_gnmt.py:280) ->
 * GNMTDecoder.decode_seq (gnmt.py:254-304).  tgt (B, ld) int32 DEVICE tokens, first `steps`
 * columns are fed; logits (B, steps, V) fp32.  Needs a preceding tn_gnmt_encode. */
int tn_gnmt_decode_seq(tn_gnmt *g, const int32_t *tgt, int ld, int steps, float *logits);
/* The decoder's attention weights, the additional outputs of GNMTDecoder(output_attention=True) (gnmt.py:302-303,402-403):
 * the scaled-Luong distribution over the T encoder steps of the last tn_gnmt_encode[_rows], exact zeros at and beyond a clip's
 * valid_len.  Both calls are their namesakes with one more DEVICE output, which must not be NULL (TN_ERR_INVALID); the
 * namesakes are the same code with no such output and launch what they always launched.
 *   tn_gnmt_decode_seq_attention   attention (B, steps, T) fp32: decode_seq stacks the steps' weights (gnmt.py:302-303).
 *   tn_gnmt_beam_search_attention  attention (B, beam, max_length + 1, T) fp32 with max_length the one given to tn_gnmt_create:
 *                                  row i of hypothesis (b, k) holds the weights of the decoder step (gnmt.py:402-403) that
 *                                  emitted samples[b, k, i + 1], followed through the beam reshuffling; rows whose token no
 *                                  decoder step emitted (the -1 padding, the <eos> appended at max_length) are zeros.
 *                                  The first call that asks allocates the steps' history inside the handle,
 *                                  4 * max_length * max_batch * beam * max_src_len bytes (61.4 MB for 150 x 32 x 5 x 640),
 *                                  released by tn_gnmt_destroy; a handle that never asks allocates nothing. */
int tn_gnmt_decode_seq_attention(tn_gnmt *g, const int32_t *tgt, int ld, int steps, float *logits, float *attention);
int tn_gnmt_beam_search_attention(tn_gnmt *g, int bos, int eos, float alpha, float K, int max_length, int32_t *samples,
                                  float *scores, int32_t *valid_length, int *length_host, float *attention);
/* MaskedSoftmaxCELoss [EXT gluonnlp] (train_gnmt.py:256,281): loss (B,) fp32. */
int tn_masked_softmax_ce(tn_ctx *ctx, const float *logits, const int32_t *labels, int ld_labels,
                         const int32_t *valid_len, int batch, int steps, int vocab, float *loss);
int tn_gnmt_destroy(tn_gnmt *g);

#ifdef __cplusplus
}
#endif
#endif /* TENNIS_HIP_H */
