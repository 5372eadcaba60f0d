/*
 * srgan_hip.h -- C ABI of libsrgan_hip.so: the MI355X (gfx950) kernels behind the
 * Style-Restricted GAN G+D+E train step.
 *
 * The reference (shinshoji01/Style-Restricted_GAN) has no FFI layer: its "operator API" is
 * the set of torch.nn / torch.nn.functional calls made by pyfiles/model.py, pyfiles/util.py
 * and pyfiles/util_notebook.py.  Each entry point below names the reference call site(s) it
 * replaces.  The Python host (style-restricted_gan_amd/srgan_amd) binds these with ctypes and
 * mirrors the reference's nn.Module / loss / trainer signatures on top of them.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to dense fp32 data unless stated otherwise;
 *   - activations are NHWC ([N][H][W][C], C fastest); 2-D tensors are row-major;
 *   - conv weights are read through explicit element strides (sO,sI,sH,sW) of the logical
 *     [O][I][kh][kw] tensor, so PyTorch's OIHW parameters are consumed in place;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing syncs;
 *   - `ws` / `ws_bytes`: caller-owned scratch, size from the matching *_workspace() query;
 *   - return value: 0 on success, <0 invalid argument, >0 a hipError_t.  The text of the last
 *     error of the calling thread is available from srgan_last_error().
 */
#ifndef SRGAN_HIP_H
#define SRGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRGAN_ABI_VERSION 1

enum { SRGAN_ACT_NONE = 0, SRGAN_ACT_RELU = 1, SRGAN_ACT_LRELU = 2 };
enum { SRGAN_PAD_ZERO = 0, SRGAN_PAD_REFLECT = 1 };
/* criterion kind of the fused loss kernels: nn.MSELoss, or the binary cross-entropy of the slot (nn.BCEWithLogitsLoss on the
 * discriminator's raw maps, nn.BCELoss on the class probabilities); mean reduction, no weights */
enum { SRGAN_CRIT_MSE = 0, SRGAN_CRIT_BCE = 1 };

int srgan_abi_version(void);
const char* srgan_last_error(void);

/* Geometry of one convolution y[N,Ho,Wo,O] = conv(x[N,Hi,Wi,I], w[O,I,kh,kw]) (+bias). */
typedef struct srgan_conv_desc {
  int N, Hi, Wi, I;      /* input  */
  int Ho, Wo, O;         /* output */
  int kh, kw, stride, pad;
  int pad_mode;          /* SRGAN_PAD_* (reflect: pyfiles/model.py:358,364,419,425) */
  long long sO, sI, sH, sW; /* element strides of the logical [O][I][kh][kw] weight */
} srgan_conv_desc;

/* nn.Conv2d forward (pyfiles/model.py:191,193,212,215,232,262,269,302,309,328-331,358,364,
 * 369,385,445) with optional bias and fused activation epilogue (nn.LeakyReLU model.py:263).
 * Also the input-gradient of nn.ConvTranspose2d (model.py:227,230) when called with the
 * transposed-conv weight viewed as [O=Cin_t][I=Cout_t]. */
size_t srgan_conv2d_workspace(const srgan_conv_desc* d);
int srgan_conv2d_fwd(const srgan_conv_desc* d, const float* x, const float* w, const float* bias,
                     float* y, int act, float slope, void* ws, size_t ws_bytes, void* stream);

/* Gradient w.r.t. the conv input (autograd of the call sites above): dx[N,Hi,Wi,I].
 * Also the FORWARD of nn.ConvTranspose2d (model.py:227,230).  Weights are read at call time. */
int srgan_conv2d_dgrad(const srgan_conv_desc* d, const float* dy, const float* w, float* dx,
                       void* ws, size_t ws_bytes, void* stream);

/* Packed-weight variants: the repacked weight operand ([phase][Npad][Kpad], or the narrow-output layout) depends only
 * on (desc, kind, act); pack it once per optimiser step and reuse it for every forward (kind 0) / input-gradient
 * (kind 1) of that step.  srgan_conv2d_fwd / _dgrad are exactly pack-into-workspace + the packed call. */
size_t srgan_conv2d_packed_bytes(const srgan_conv_desc* d, int kind, int act);
int srgan_conv2d_pack(const srgan_conv_desc* d, int kind, int act, const float* w, void* packed, size_t bytes, void* stream);
/* Scratch the packed calls need beside the operand (0 for most layers): the transformed-input image of the F(4x4,3x3)
 * Winograd layers (kind 0 and 1), the padded-gradient temp of a reflect-padded layer (kind 1).  Caller-owned like every
 * workspace of this library; only live between the launches of one call, so one buffer serves every layer of a stream. */
size_t srgan_conv2d_packed_scratch(const srgan_conv_desc* d, int kind);
/* Non-zero when the packed operand depends on the weights and channel counts only (Winograd filter images, RGB-input image):
 * descriptors of the same weight that differ in N / H / W only and return the same signature may share one packed buffer. */
unsigned long long srgan_conv2d_pack_signature(const srgan_conv_desc* d, int kind, int act);
int srgan_conv2d_fwd_packed(const srgan_conv_desc* d, const float* x, const void* packed, const float* bias, float* y,
                            int act, float slope, void* ws, size_t ws_bytes, void* stream);
int srgan_conv2d_dgrad_packed(const srgan_conv_desc* d, const float* dy, const void* packed, float* dx,
                              void* ws, size_t ws_bytes, void* stream);
/* conv3x3(act(instance_norm(x) * scale + shift)) without the intermediate tensor: inside SingleResidualBlock (model.py:196-201:
 * c1 -> cn1 -> ReLU -> c2) the normalised activation is read by c2 only.  srgan_instnorm_fwd_v = srgan_instnorm_fwd (same
 * statistics, same expression, mean / rstd saved for the backward) whose output is written directly as the transformed-input
 * ("V") image of the F(4x4,3x3) layer `d` (v_bytes >= srgan_conv2d_packed_scratch(d, 0)); srgan_conv2d_fwd_from_v then runs
 * that layer's multiply + output transform on it, and srgan_conv2d_wgrad_v its weight gradient.  Applicable
 * (srgan_instnorm_conv_v_applicable != 0) to 32x32 maps with Cin % 32 == 0 whose forward dispatches to F(4x4,3x3). */
int srgan_instnorm_conv_v_applicable(const srgan_conv_desc* d);
int srgan_instnorm_fwd_v(const srgan_conv_desc* d, const float* x, const float* scale, const float* shift, float* mean,
                         float* rstd, void* v_image, size_t v_bytes, float eps, int act, float slope, void* stream);
int srgan_conv2d_fwd_from_v(const srgan_conv_desc* d, const void* v_image, const void* packed, const float* bias, float* y,
                            int act, float slope, void* stream);
/* The backward counterpart.  `d` describes a convolution whose OUTPUT y is normalised (y -> (CB)IN -> activation): the gradient
 * dy w.r.t. y, produced by the norm's backward, is read by exactly two kernels -- the convolution's input gradient and its
 * F(4x4,3x3) weight gradient -- each through a transform.  srgan_instnorm_bwd_vz = srgan_instnorm_bwd (same dscale / dshift,
 * same dy values) that writes those two transforms instead of dy: v_image (srgan_conv2d_packed_scratch(d, 1) bytes) for
 * srgan_conv2d_dgrad_from_v (multiply + output transform, optional skip-path gradient `res` as in ..._dgrad_packed_add), z_image
 * (srgan_instnorm_bwd_vz_z_bytes(d) bytes) for srgan_conv2d_wgrad_vz (with the V image the forward kept).  x = y (the conv
 * output the forward normalised), dy = gradient w.r.t. the norm's output. */
int srgan_instnorm_bwd_vz_applicable(const srgan_conv_desc* d);
size_t srgan_instnorm_bwd_vz_z_bytes(const srgan_conv_desc* d);
int srgan_instnorm_bwd_vz(const srgan_conv_desc* d, const float* x, const float* dy, const float* scale, const float* shift,
                          const float* mean, const float* rstd, float* dscale, float* dshift, void* v_image, size_t v_bytes,
                          void* z_image, size_t z_bytes, int act, float slope, void* stream);
int srgan_conv2d_dgrad_from_v(const srgan_conv_desc* d, const void* v_image, const void* packed, const float* res, float* dx,
                              void* stream);
int srgan_conv2d_wgrad_vz(const srgan_conv_desc* d, const float* v_image, const float* z_image, float* dw, void* ws,
                          size_t ws_bytes, void* stream);
/* dx = (input gradient of the convolution) + res: SingleResidualBlock (model.py:196-201) feeds its input to its first
 * convolution AND to the skip connection, so the gradient of the block input is the sum of the two paths; handing the skip
 * path's gradient to the convolution's input-gradient kernel (added in the F(4x4,3x3) epilogue; one in-place pass on the other
 * dispatches) replaces autograd's separate accumulation pass over the tensor.  res: dense, shape of dx, must not alias dx. */
/* dx = (input gradient of the convolution) * LeakyReLU'(mask): a discriminator trunk is conv -> LeakyReLU(0.2) -> conv -> ...
 * (model.py:303-309), so the gradient this layer hands to the previous one must still be multiplied by that layer's LeakyReLU
 * derivative -- 1 or `slope` after the sign of its activated output, which IS this layer's input tensor (`mask`).  Folded into
 * the epilogue of the transposed F(3x3,2x2) kernel (one in-place elementwise pass on the other dispatches) it replaces the
 * read-read-write pass in front of the previous layer's backward.  mask: dense, shape of dx, must not alias dx. */
int srgan_conv2d_dgrad_packed_mask(const srgan_conv_desc* d, const float* dy, const void* packed, const float* mask, float slope,
                                   float* dx, void* ws, size_t ws_bytes, void* stream);
int srgan_conv2d_dgrad_packed_add(const srgan_conv_desc* d, const float* dy, const void* packed, const float* res, float* dx,
                                  void* ws, size_t ws_bytes, void* stream);

/* Many packs in one launch (after an optimiser step every cached operand of the network is stale at once):
 * srgan_conv2d_pack_entry writes one host record (srgan_pack_entry_bytes() bytes) per operand -- it returns 1 for the few
 * layers whose operand is made by another kernel (narrow-output layers; use srgan_conv2d_pack) -- the caller copies the array
 * of records to the device and srgan_conv2d_pack_multi repacks them all. */
size_t srgan_pack_entry_bytes(void);
int srgan_conv2d_pack_entry(const srgan_conv_desc* d, int kind, int act, const float* w, void* packed, void* entry);
int srgan_conv2d_pack_multi(const void* entries_dev, int n_entries, void* stream);

/* Gradient w.r.t. the conv weight, written through (sO,sI,sH,sW); dbias[O] (may be NULL) = column sums of dy.
 * Overwrites dw / dbias, unless srgan_set_wgrad_accumulate(1) is in effect on the calling host thread: then every weight-gradient
 * entry point (srgan_conv2d_wgrad, _wgrad_v, _wgrad_vz, srgan_halo16_wgrad) ADDS its result in the split-K slab reduce
 * (dw += ...): the reference's autograd sums the two uses of the generator's weights inside one backward call
 * (util_notebook.py:664, :689; torch's AccumulateGrad input buffer) -- here without a separate elementwise pass. */
int srgan_set_wgrad_accumulate(int on);

/* Deferred slab sums (round 3).  Every weight-gradient entry point ends in a split-K slab sum of ~12 us that cannot fill the
 * chip; the reference's step has 145 of them.  Between srgan_wgrad_defer_begin(arena, bytes) and srgan_wgrad_defer_end()
 * (process-wide -- autograd calls the entry points from its own thread -- so one backward pass at a time) a call made with bit 1 of the switch above set -- srgan_set_wgrad_accumulate(2 | accumulate): "nobody reads dw
 * before _end", true for the gradient buffers autograd's AccumulateGrad (util_notebook.py:664, :689 `.backward()`) would fill --
 * takes its workspace from the arena (256-byte aligned device memory, the caller keeps it alive and untouched until _end; `ws`
 * is then unused) and queues its sum; queued sums run as ONE launch when 40 are waiting, when the arena is full, when a second
 * sum for the same dw arrives, and at _end -- all on `stream`; calls made on any other stream are not deferred.  Same per-output loop and rounding as the
 * immediate sums: identical bits.  dbias column sums are not deferred. */
int srgan_wgrad_defer_begin(void* arena, size_t arena_bytes, void* stream);
int srgan_wgrad_defer_end(void);
/* Process totals since load: slab sums that went through the queue, and the launches that ran them. */
int srgan_wgrad_defer_stats(long long* sums, long long* launches);
/* Workspace bytes the deferrable calls since the last srgan_wgrad_defer_begin asked for (whether or not they fitted): an arena
 * of that size holds a whole pass without an early flush -- the caller sizes it from its first pass instead of guessing. */
int srgan_wgrad_defer_need(long long* bytes);
int srgan_conv2d_wgrad(const srgan_conv_desc* d, const float* x, const float* dy, float* dw,
                       float* dbias, void* ws, size_t ws_bytes, void* stream);

/* The same gradient from the transformed input the FORWARD of an F(4x4,3x3) layer already wrote (pyfiles/model.py:191,193: the
 * residual-trunk convs): when srgan_conv2d_wgrad_v_bytes(d) != 0, hand srgan_conv2d_fwd_packed a buffer of that many bytes as
 * `ws` and keep it until the backward pass; srgan_conv2d_wgrad_v then needs neither x nor a second input transform. */
size_t srgan_conv2d_wgrad_v_bytes(const srgan_conv_desc* d);
int srgan_conv2d_wgrad_v(const srgan_conv_desc* d, const float* v_image, const float* dy, float* dw,
                         float* dbias, void* ws, size_t ws_bytes, void* stream);

/* Instance norm + per-(n,c) affine + activation (+ residual):
 *   xh = (x - mean_nc) * rstd_nc ; y = act(xh * scale[n,c] + shift[n,c]) (+ res)
 * F.instance_norm(eps=1e-5, biased var) at model.py:58-60 (CBIN), nn.InstanceNorm2d at
 * model.py:178 (scale/shift NULL), nn.ReLU model.py:199,240,246, LeakyReLU(0.2) model.py:418,
 * residual add model.py:201.  mean/rstd [N*C] are written for the backward. */
size_t srgan_instnorm_workspace(int N, int HW, int C);
int srgan_instnorm_fwd(const float* x, const float* scale, const float* shift, const float* res,
                       float* y, float* mean, float* rstd, int N, int HW, int C, float eps,
                       int act, float slope, void* ws, size_t ws_bytes, void* stream);
/* Backward: dx, and (when scale!=NULL or wanted) dscale[n,c]=sum dy_act*xh, dshift[n,c]=sum dy_act.
 * dres is dy itself (caller aliases it).  y_act_src: the forward's x (pre-norm) is re-normalised
 * to rebuild the activation mask. */
int srgan_instnorm_bwd(const float* x, const float* dy, const float* scale, const float* shift,
                       const float* mean, const float* rstd, float* dx, float* dscale,
                       float* dshift, int N, int HW, int C, int act, float slope,
                       void* ws, size_t ws_bytes, void* stream);

/* Batch normalisation + activation (+ residual), norm_type="batch" (model.py:173-176).  NHWC fp32, C % 4 == 0.
 *   BN  (nn.BatchNorm2d(C, affine=True), model.py:175; the encoder blocks' norm1 / norm2, model.py:404-408, and the
 *        generator's up-path norms, model.py:236-246):  y = act((x - mu_c) * r_c * weight + bias)
 *   CBB (CBBNorm2d, model.py:75-171; F.batch_norm then out - avgpool(out) + tanh(Linear(c)), model.py:118-140):
 *        y = act((x - mu_nc) * r_c * scale[n,c] + shift[n,c]) (+ res), scale / shift from srgan_cbin_affine_fwd
 * mu_c / var_c: biased batch statistics over (n, h, w); mu_nc: the image's channel mean; r_c = (var_c + eps)^-1/2.
 * training != 0: batch statistics; with running_mean / running_var given they are updated on the device
 *   (running = (1 - f) * running + f * stat, the variance unbiased by M / (M - 1), M = N * HW) and num_batches_tracked
 *   (int64, may be null unless cumulative) is advanced; f = momentum, or 1 / num_batches_tracked when cumulative
 *   (momentum=None), read on the device.  training == 0: running_mean / running_var stand in (required).  M <= 1 in
 *   training is an error ("Expected more than 1 value per channel when training", F.batch_norm).
 * Outputs kept for the backward: mean / rstd [C] (the statistics used), m / a / b [N*C] (y = act((x - m) * a + b)).
 * Deterministic: fixed-order reductions, no atomics.  ws: srgan_batchnorm_workspace(N, HW, C) bytes (forward and backward). */
size_t srgan_batchnorm_workspace(int N, int HW, int C);
int srgan_batchnorm_fwd(const float* x, const float* weight, const float* bias, float* y, float* mean, float* rstd,
                        float* m, float* a, float* b, float* running_mean, float* running_var,
                        long long* num_batches_tracked, int N, int HW, int C, int training, float momentum,
                        int cumulative, float eps, int act, float slope, void* ws, size_t ws_bytes, void* stream);
int srgan_cbbnorm_fwd(const float* x, const float* scale, const float* shift, const float* res, float* y, float* mean,
                      float* rstd, float* m, float* a, float* b, float* running_mean, float* running_var,
                      long long* num_batches_tracked, int N, int HW, int C, int training, float momentum,
                      int cumulative, float eps, int act, float slope, void* ws, size_t ws_bytes, void* stream);
/* Backward from the forward's mean / rstd / m / a / b (the activation mask is rebuilt from x): dx, and dweight / dbias [C]
 * (BN) or dscale / dshift [N*C] (CBB, into srgan_cbin_affine_bwd).  training: the forward used batch statistics
 * (autograd of F.batch_norm, model.py:130-132 and nn.BatchNorm2d); otherwise r_c is a constant.  dres is dy itself.
 * BN: `weight` (may be null: 1) is read when the backward RUNS -- nn.BatchNorm2d's autograd holds it by reference, so a
 * backward through a graph recorded before an optimiser step sees the updated weight (the reference's train step does this,
 * util_notebook.py:664-690); CBB's scale is the forward-time affine (model.py:136-138 multiplies by a weight.repeat copy). */
int srgan_batchnorm_bwd(const float* x, const float* dy, const float* weight, const float* mean, const float* rstd,
                        const float* m, const float* a, const float* b, float* dx, float* dweight, float* dbias, int N,
                        int HW, int C, int training, int act, float slope, void* ws, size_t ws_bytes, void* stream);
int srgan_cbbnorm_bwd(const float* x, const float* dy, const float* scale, const float* mean, const float* rstd,
                      const float* m, const float* a, const float* b, float* dx, float* dscale, float* dshift, int N,
                      int HW, int C, int training, int act, float slope, void* ws, size_t ws_bytes, void* stream);

/* The same norms under data parallelism, with the statistics of the GLOBAL batch (training mode only).  This rank holds images
 * [n0, n0 + N_local) of N_global, n0 = rank * N_local.  Each direction is split around one all-gather that the caller issues
 * between the two calls (srgan_allgather_rows or any other transport), in place on the exchange buffer `xbuf`:
 *   *_partial : this rank's per-(image, slab, channel) partials, with the slab plan of the GLOBAL batch, into its chunk of xbuf;
 *   all-gather: chunk r of xbuf (xbuf_bytes / (N_global / N_local) bytes each) comes from rank r;
 *   *_apply   : the one-process merge over all N_global images in the one-process order, then the elementwise pass on the local
 *               images.  mean / rstd, the running buffers, y and dx are bit-identical to one process with N_global images.
 * xbuf: srgan_batchnorm_sync_exchange_bytes(N_global, N_local, HW, C, with_scale) bytes, fp32; with_scale = 1 for the CBB
 * backward (the chunk then ends in the rank's scale rows, which the other ranks' delta needs), 0 otherwise.  The backward's
 * parameter gradients are sums over the LOCAL images (the gradient all-reduce averages them over the ranks); only the dx
 * coefficients use the global sums.  x / y / dy / dx / res and m / a / b / scale / shift / dscale / dshift are the local
 * images'.  ws (backward apply): srgan_batchnorm_sync_workspace(N_local, C) bytes.  Everything else as above. */
size_t srgan_batchnorm_sync_exchange_bytes(int N_global, int N_local, int HW, int C, int with_scale);
size_t srgan_batchnorm_sync_workspace(int N_local, int C);
int srgan_batchnorm_sync_fwd_partial(const float* x, void* xbuf, size_t xbuf_bytes, int N_global, int n0, int N_local, int HW,
                                     int C, void* stream);
int srgan_batchnorm_sync_fwd_apply(const float* x, const float* weight, const float* bias, float* y, float* mean, float* rstd,
                                   float* m, float* a, float* b, float* running_mean, float* running_var,
                                   long long* num_batches_tracked, const void* xbuf, size_t xbuf_bytes, int N_global, int n0,
                                   int N_local, int HW, int C, float momentum, int cumulative, float eps, int act, float slope,
                                   void* stream);
int srgan_cbbnorm_sync_fwd_apply(const float* x, const float* scale, const float* shift, const float* res, float* y,
                                 float* mean, float* rstd, float* m, float* a, float* b, float* running_mean,
                                 float* running_var, long long* num_batches_tracked, const void* xbuf, size_t xbuf_bytes,
                                 int N_global, int n0, int N_local, int HW, int C, float momentum, int cumulative, float eps,
                                 int act, float slope, void* stream);
/* scale: CBB's [N_local * C] affine (then xbuf has the with_scale layout), null for BN */
int srgan_batchnorm_sync_bwd_partial(const float* x, const float* dy, const float* scale, const float* rstd, const float* m,
                                     const float* a, const float* b, void* xbuf, size_t xbuf_bytes, int N_global, int n0,
                                     int N_local, int HW, int C, int act, float slope, void* stream);
int srgan_batchnorm_sync_bwd_apply(const float* x, const float* dy, const float* weight, const float* mean, const float* rstd,
                                   const float* m, const float* a, const float* b, const void* xbuf, size_t xbuf_bytes,
                                   float* dx, float* dweight, float* dbias, int N_global, int n0, int N_local, int HW, int C,
                                   int act, float slope, void* ws, size_t ws_bytes, void* stream);
int srgan_cbbnorm_sync_bwd_apply(const float* x, const float* dy, const float* mean, const float* rstd, const float* m,
                                 const float* a, const float* b, const void* xbuf, size_t xbuf_bytes, float* dx, float* dscale,
                                 float* dshift, int N_global, int n0, int N_local, int HW, int C, int act, float slope, void* ws,
                                 size_t ws_bytes, void* stream);

/* Central-biasing affine of _CBINorm.forward (model.py:54-67): t = tanh(c W^T + b);
 * scale[n,ch] = gamma[ch]; shift[n,ch] = t*gamma + beta.  c:[N,num_con] W:[C,num_con]. */
int srgan_cbin_affine_fwd(const float* c, const float* W, const float* b, const float* gamma,
                          const float* beta, float* t, float* scale, float* shift,
                          int N, int C, int num_con, void* stream);
/* Backward of the above from dscale/dshift[N,C]: dgamma, dbeta, dW, db (overwritten), dc [N,num_con]. */
int srgan_cbin_affine_bwd(const float* c, const float* W, const float* gamma, const float* t,
                          const float* dscale, const float* dshift, float* dgamma, float* dbeta,
                          float* dW, float* db, float* dc, int N, int C, int num_con,
                          void* ws, size_t ws_bytes /* >= N*C floats */, void* stream);

/* The same affine for ALL central-biasing layers of a network in one launch (forward) / two launches (backward): the 15
 * `_CBINorm` layers of SingleGenerator (model.py:213-224) depend on the style code and their own parameters only.
 * The caller fills one host record per layer (srgan_cbin_rec_bytes() bytes each; pointers a pass does not use may be NULL),
 * copies the array to the device and passes it as `table_dev`; outputs of a layer are dense [N][C] blocks.
 * Backward: dscale / dshift must be non-NULL (zeros for absent gradients), `da` is [N][C] scratch per layer, `gamma` is the
 * forward-time copy (row 0 of the saved scale); dc[N][num_con] sums the layers in table order (dc may be NULL: the style
 * code's gradient is only wanted when the code came from the encoder, not for the noise codes of most generator passes). */
size_t srgan_cbin_rec_bytes(void);
int srgan_cbin_rec_fill(void* rec, const float* W, const float* b, const float* gamma, const float* beta, float* t,
                        float* scale, float* shift, const float* dscale, const float* dshift, float* dgamma,
                        float* dbeta, float* dW, float* db, float* da, int C);
/* on != 0: the backward of this record ADDS to dgamma / dbeta / dW / db (a layer reached twice in one backward pass: the
 * generator is back-propagated through two graphs inside util_notebook.py:664 and again inside :689). */
int srgan_cbin_rec_set_accumulate(void* rec, int on);
int srgan_cbin_affine_multi_fwd(const float* c, const void* table_dev, int n_layers, int N, int max_C, int num_con,
                                void* stream);
int srgan_cbin_affine_multi_bwd(const float* c, const void* table_dev, int n_layers, int N, int max_C, int num_con,
                                float* dc, void* stream);

/* Pointwise: y = act(x) and dx = dy * act'(y) (mask from the OUTPUT sign, slope>0). tanh: model.py:248 */
int srgan_act_fwd(const float* x, float* y, long long n, int act, float slope, void* stream);
int srgan_act_bwd(const float* y, const float* dy, float* dx, long long n, int act, float slope, void* stream);
int srgan_tanh_fwd(const float* x, float* y, long long n, void* stream);
int srgan_tanh_bwd(const float* y, const float* dy, float* dx, long long n, void* stream);
/* y = a + b (E block: cmp(...) + shortcut(x), model.py:436) */
int srgan_add(const float* a, const float* b, float* y, long long n, void* stream);

/* nn.AvgPool2d(3, stride=2, padding=1, count_include_pad=False)  model.py:286,324 */
int srgan_avgpool3s2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int srgan_avgpool3s2_bwd(const float* dy, float* dx, int N, int H, int W, int C, void* stream);
/* nn.AvgPool2d(2,2) (floor)  model.py:365,368,426,429 */
int srgan_avgpool2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int srgan_avgpool2_bwd(const float* dy, float* dx, int N, int H, int W, int C, void* stream);
/* The same with an fp32 or bf16 tensor on either side (C % 4 == 0): around the 16-bit convolutions of the style encoder in the
 * bf16 mode (pyfiles/model.py:409-411). */
int srgan_avgpool2_fwd_io(const void* x, int x_bf16, void* y, int y_bf16, int N, int H, int W, int C, void* stream);
int srgan_avgpool2_bwd_io(const void* dy, int dy_bf16, void* dx, int dx_bf16, int N, int H, int W, int C, void* stream);
/* LeakyReLU(slope) -> AdaptiveAvgPool2d(1)  (Encoder.last_layer, model.py:454,475-480) */
int srgan_lrelu_gap_fwd(const float* x, float* y, int N, int HW, int C, float slope, void* stream);
int srgan_lrelu_gap_bwd(const float* x, const float* dy, float* dx, int N, int HW, int C, float slope, void* stream);

/* Encoder.reparametrize (model.py:459-463): out = eps * exp(logvar / 2) + mu, stdv = exp(logvar / 2) (kept for the backward);
 * backward: dmu = g, dlogvar = g * eps * stdv / 2.  n = B * ndim; every operation rounded on its own, as the reference's chain. */
int srgan_reparam_fwd(const float* mu, const float* logvar, const float* eps, float* out, float* stdv, long long n, void* stream);
int srgan_reparam_bwd(const float* g, const float* eps, const float* stdv, float* dlogvar, long long n, void* stream);

/* nn.Linear: y[M,N] = x[M,K] W[N,K]^T + b  (model.py:455-457; small M) */
int srgan_linear_fwd(const float* x, const float* W, const float* b, float* y, int M, int N, int K, void* stream);
int srgan_linear_bwd(const float* x, const float* W, const float* dy, float* dx, float* dW, float* db,
                     int M, int N, int K, void* stream);

/* bf16 compute mode, residual-trunk layers (3x3 / stride 1 / zero pad 1, Cin = Cout in {64, 128, 256}, maps of whole 4 x 32
 * patches; reference pyfiles/model.py:188-201) with bf16 TENSORS in HBM on either side: the kernels of the fused residual block
 * whose intermediates -- conv outputs, the normalised activation, the gradients between the norm and conv backward kernels --
 * are stored as bf16 (fp32 accumulation, fp32 statistics, fp32 master weights and residual stream).  `*_bf16` flags say which
 * side is bf16 ([N][H][W][C] dense NHWC either way).  `packed`: the ordinary packed operand of (d, kind) made in bf16 mode.
 * srgan_halo16_conv: kind 0 forward, kind 1 input gradient (+ `res`, fp32, added to an fp32 result).  srgan_halo16_wgrad: dw
 * (fp32, through the descriptor's weight strides); bf16 x requires bf16 dy.  ws: srgan_conv2d_workspace(d) bytes. */
int srgan_halo16_applicable(const srgan_conv_desc* d);
/* Round 4: the same two entry points also serve the 4x4 / stride-2 / pad-1 layers whose three directions run on the
 * LDS-resident-patch kernels in the bf16 mode -- (Cin, Cout) = (64, 128) / (128, 256), output maps of whole 4 x 32 patches: the
 * generator's down convolutions (pyfiles/model.py:212-215) and, through their transposed form, its up convolutions (:227-230).
 * kind 0 = strided form (x -> y, or a ConvTranspose2d's input gradient), kind 1 = transposed form (dy -> dx, or a ConvTranspose2d
 * forward); no `res`.  srgan_halo16_wgrad on these layers: bf16 x with fp32 or bf16 dy, or both fp32. */
int srgan_halo16s2_applicable(const srgan_conv_desc* d);
int srgan_halo16_conv(const srgan_conv_desc* d, int kind, const void* src, int src_bf16, const void* packed, const float* res,
                      void* dst, int dst_bf16, void* stream);
int srgan_halo16_wgrad(const srgan_conv_desc* d, const void* x, int x_bf16, const void* dy, int dy_bf16, float* dw, void* ws,
                       size_t ws_bytes, void* stream);
/* Round 5: the generic layers of the bf16 mode (no LDS-resident-patch kernel: the style encoder's 3x3 reflect-padded
 * convolutions on 62 / 31 / 15 / 7-pixel maps, pyfiles/model.py:413-437) with bf16 TENSORS on either side.  srgan_igemm16_io_applicable:
 * forward (with `act`), input gradient and weight gradient of d all run on the 64-deep-K-tile implicit GEMM and the vector
 * weight-gradient kernel (bf16 mode, Cin % 64 == 0, Cout % 64 == 0 ...).  srgan_igemm16_conv: kind 0 forward (bias / activation as
 * srgan_conv2d_fwd_packed), kind 1 input gradient (no bias / activation; reflect padding folds into dst's type); `packed`: the
 * ordinary packed operand of (d, kind, act); ws: srgan_conv2d_packed_scratch(d, kind) bytes.  srgan_igemm16_wgrad: x and dy both
 * bf16, dw fp32 through the descriptor's weight strides; ws: srgan_conv2d_workspace(d) bytes; honours
 * srgan_set_wgrad_accumulate / the deferred slab sums like srgan_conv2d_wgrad. */
int srgan_igemm16_io_applicable(const srgan_conv_desc* d, int act);
int srgan_igemm16_conv(const srgan_conv_desc* d, int kind, const void* src, int src_bf16, const void* packed, const float* bias,
                       void* dst, int dst_bf16, int act, float slope, void* ws, size_t ws_bytes, void* stream);
int srgan_igemm16_wgrad(const srgan_conv_desc* d, const void* x, const void* dy, float* dw, void* ws, size_t ws_bytes, void* stream);
/* bf16 mode, round 6: the 4x4 / stride-2 / pad-1 layers of the discriminator trunks (pyfiles/model.py:302-309: conv without bias
 * -> LeakyReLU(0.01), no norm between the layers) with bf16 tensors on either side: forward with the bias / activation epilogue
 * (halo16s_kernel, or igemm16_kernel with LDS-DMA tiles), input gradient (halo16t_kernel or igemm16_kernel); the weight gradient is
 * srgan_halo16_wgrad.  `packed`: the ordinary packed operand of (d, kind, act).  ws: srgan_conv2d_packed_scratch(d, kind) bytes. */
/* Also (act = none): the generator's 7x7 / stride-1 / pad-3 layers between a 3-channel and a 64-channel tensor (pyfiles/model.py:212,
 * 232) with the 64-CHANNEL side in bf16 -- the RGB input layer writes a bf16 y and takes a bf16 dy, the RGB output layer reads a
 * bf16 x and writes a bf16 dx; the 3-channel side is fp32 (a bf16 flag there is refused).  Their weight gradient is
 * srgan_halo16_wgrad too (bf16 allowed on the 64-channel tensor only). */
int srgan_conv2d_io_applicable(const srgan_conv_desc* d, int act);
int srgan_conv2d_io_fwd(const srgan_conv_desc* d, const void* x, int x_bf16, const void* packed, const float* bias, void* y, int y_bf16,
                        int act, float slope, void* ws, size_t ws_bytes, void* stream);
int srgan_conv2d_io_dgrad(const srgan_conv_desc* d, const void* dy, int dy_bf16, const void* packed, void* dx, int dx_bf16, void* ws,
                          size_t ws_bytes, void* stream);
/* LeakyReLU / ReLU backward dx = dy * f'(y) over n elements (n % 8 == 0), every tensor fp32 or bf16 (nn.LeakyReLU, model.py:303,310). */
int srgan_act_bwd_io(const void* y, int y_bf16, const void* dy, int dy_bf16, void* dx, int dx_bf16, long long n, int act, float slope,
                     void* stream);
/* Single-pass instance norm (+ per-sample scale / shift, activation, optional fp32 skip tensor) of maps with <= 1024 pixels with
 * bf16 tensors on either side; statistics, sums, scale / shift gradients in fp32.  Backward: x = the normalised tensor's INPUT
 * (fp32 or bf16), dy fp32 or bf16, dx of x's type.  srgan_instnorm_slab_applicable: the shape is served (C % 32 == 0, HW <= 1024, enough slabs). */
int srgan_instnorm_slab_applicable(int N, int HW, int C);
int srgan_instnorm_slab_fwd_io(const void* x, int x_bf16, const float* scale, const float* shift, const float* res, void* y,
                               int y_bf16, float* mean, float* rstd, int N, int HW, int C, float eps, int act, float slope,
                               void* stream);
int srgan_instnorm_slab_bwd_io(const void* x, int x_bf16, const void* dy, int dy_bf16, const float* scale, const float* shift,
                               const float* mean, const float* rstd, void* dx, int dx_bf16, float* dscale, float* dshift, int N,
                               int HW, int C, int act, float slope, void* stream);
/* Instance norm (+ affine, activation) with fp32 or bf16 tensors on either side, for the shapes the slab kernels or the fast
 * two-pass kernels serve (srgan_instnorm_io_applicable: HW <= 1024 with C % 32 == 0, or C | 1024 with C % 4 == 0): the norms
 * between the generator's down / up convolutions when the bf16 mode keeps those activations in 16 bits (pyfiles/model.py:54-67,
 * 228, 231, 245-246) and, on maps too large for the slab kernels, the norms inside a residual block with bf16 intermediates
 * (`res`: fp32 skip tensor added to an fp32 result; pyfiles/model.py:86-94).  Statistics, scale / shift and their gradients are
 * fp32.  Backward: dx has x's type.  ws:
 * srgan_instnorm_workspace(N, HW, C) bytes. */
int srgan_instnorm_io_applicable(int N, int HW, int C);
int srgan_instnorm_fwd_io(const void* x, int x_bf16, const float* scale, const float* shift, const float* res, void* y, int y_bf16,
                          float* mean, float* rstd, int N, int HW, int C, float eps, int act, float slope, void* ws, size_t ws_bytes,
                          void* stream);
int srgan_instnorm_bwd_io(const void* x, int x_bf16, const void* dy, int dy_bf16, const float* scale, const float* shift,
                          const float* mean, const float* rstd, void* dx, int dx_bf16, float* dscale, float* dshift, int N, int HW,
                          int C, int act, float slope, void* ws, size_t ws_bytes, void* stream);

/* NCHW <-> NHWC repack at the module boundary. */
int srgan_nchw_to_nhwc(const float* x, float* y, int N, int C, int H, int W, void* stream);
int srgan_nhwc_to_nchw(const float* x, float* y, int N, int C, int H, int W, void* stream);

/* ---- fused loss reductions (value + gradient in one launch) -------------------------------
 * Each writes loss[0] (overwrite) and the gradient of `weight * loss` w.r.t. its input. */
/* get_loss_D, util.py:457-462 with nn.MSELoss: one scale; loss = mean((o-target)^2)*weight */
int srgan_mse_const(const float* o, long long n, float target, float weight, float* loss, float* d_o, void* stream);
/* get_loss_D, util.py:457-462 (`criterion(output, targets)` with targets = full_like(output, target)) for either criterion
 * kind: SRGAN_CRIT_MSE is srgan_mse_const; SRGAN_CRIT_BCE is nn.BCEWithLogitsLoss on the raw map,
 * loss = weight * mean(max(o,0) - o*target + log1p(exp(-|o|))), d_o = weight * (sigmoid(o) - target) / n; any real target. */
int srgan_crit_const(const float* o, long long n, float target, float weight, int kind, float* loss, float* d_o, void* stream);
/* nn.Softmax(dim=1) + get_domainloss_D (util.py:464-468, model.py:333-346): z:[B,n_class] logits,
 * label:[B] int64; q=softmax(z) is written to `q`; loss = mean((q-onehot)^2)*weight; dz via softmax Jacobian. */
int srgan_softmax_mse(const float* z, const long long* label, int B, int n_class, float weight,
                      float* q, float* loss, float* dz, void* stream);
/* nn.Softmax(dim=1) + get_domainloss_D (util.py:464-468: `criterion_class(output_class, true_label)`, model.py:333-346) for
 * either kind: SRGAN_CRIT_MSE is srgan_softmax_mse; SRGAN_CRIT_BCE is nn.BCELoss(q, onehot(label)) with ATen's -100 clamp of
 * both logs and its 1e-12 floor under q (1 - q) in the gradient (a saturated row: element losses of 100, dz = 0). */
int srgan_softmax_crit(const float* z, const long long* label, int B, int n_class, float weight, int kind,
                       float* q, float* loss, float* dz, void* stream);
/* nn.CrossEntropyLoss() (mean reduction) of the encoder pre-training job, 04_Facial_Recognition-Encoder.ipynb cell 18/22:
 * loss = weight * mean_b(logsumexp(z_b) - z_b[label_b]); dz = weight * (softmax(z) - onehot) / B. */
int srgan_softmax_xent(const float* z, const long long* label, int B, int n_class, float weight, float* loss,
                       float* dz, void* stream);
/* torch.mean(torch.abs(a-b)) util_notebook.py:625,639,676,686 ; da = weight*sign(a-b)/n, db = -da */
size_t srgan_l1_workspace(long long n);
int srgan_l1_mean(const float* a, const float* b, long long n, float weight, float* loss,
                  float* da, float* db, void* ws, size_t ws_bytes, void* stream);
/* batch-KL + correlation + histogram-imitation on mu[B,d] (util_notebook.py:644-662, util.py:470-553).
 * vals[4] = (bKL, corr, hist, w_bkl*bKL + w_corr*corr + w_hist*hist); dmu = gradient of vals[3].
 * A term whose weight is exactly 0 contributes exactly 0 to vals[3] and dmu, whatever its raw value (which vals[0..2] keep
 * reporting: it may be Inf / NaN on inputs only the other terms are asked about).
 * hist_target: [bins] device floats.  2 <= B, 2 <= d <= 16, 1 <= bins <= 64, B*d <= 16384 (one workgroup, mu staged in LDS). */
int srgan_latent_losses(const float* mu, int B, int d, float n_batch, const float* hist_target, int bins,
                        float range_max, float sigma, float w_bkl, float w_corr, float w_hist,
                        float* vals, float* dmu, float* corr_out /* [d*d] Pearson matrix or NULL */, void* stream);
/* Every loss of ONE discriminator evaluation in one launch (util.py:457-468 as used by util_notebook.py:582-590 and :622-624):
 * per scale s an LSGAN map o[s] = [rows][per_row[s]] and class logits z[s] = [rows][n_class] (z / dz may be NULL: no class
 * head).  Rows [0, rows_first) are compared with the constant t_first and carry the softmax + class-MSE loss against label[];
 * rows [rows_first, rows) (the translated half of a real | fake batch; may be empty) with t_rest.
 * vals[4] = {lsgan_first, class, lsgan_rest, total}, each the mean over scales of the per-scale nn.MSELoss,
 * total = lsgan_first + w_class * class + lsgan_rest; d_o[s] / dz[s] = d total / d o[s], z[s] (zero rows where unused).
 * o, per_row, z, d_o, dz are HOST arrays of n_scales (<= 4) entries. */
int srgan_d_losses(const float* const* o, const long long* per_row, const float* const* z, int n_scales, int rows,
                   int rows_first, int n_class, const long long* label, float t_first, float t_rest, float w_class,
                   float* vals, float* const* d_o, float* const* dz, void* stream);
/* srgan_d_losses for any pair of criterion kinds (util.py:457-468 as used by util_notebook.py:582-590 and :622-624 with the
 * trainer's `criterion` / `criterion_class`): gan_kind selects nn.MSELoss / nn.BCEWithLogitsLoss for the maps, class_kind
 * nn.MSELoss / nn.BCELoss for softmax(z) against the one-hot label; (SRGAN_CRIT_MSE, SRGAN_CRIT_MSE) is srgan_d_losses. */
int srgan_d_losses_crit(const float* const* o, const long long* per_row, const float* const* z, int n_scales, int rows,
                        int rows_first, int n_class, const long long* label, float t_first, float t_rest, float w_class,
                        int gan_kind, int class_kind, float* vals, float* const* d_o, float* const* dz, void* stream);
/* out[0] = sum_i w[i] * x[i][0] over n <= 16 device scalars (x, w: host arrays) -- the weighted sum of a phase's loss terms
 * (util_notebook.py:585, :626-662, :677-687) in one launch; srgan_lincomb_bwd: dx[i] = w[i] * g[0]. */
int srgan_lincomb(const float* const* x, const float* w, int n, float* out, void* stream);
int srgan_lincomb_bwd(const float* w, int n, const float* g, float* dx, void* stream);
/* conventional KL term of the encoder (util_notebook.py:630-634; SingleGAN: :302): weight * -0.5 * sum(1 + logvar - mu^2 -
 * exp(logvar)) over all n = B*ndim values, with dmu / dlogvar (either may be NULL) in the same launch */
int srgan_kl_normal(const float* mu, const float* logvar, long long n, float weight, float* loss, float* dmu,
                    float* dlogvar, void* stream);
/* generic nn.MSELoss(a, b) * weight with both gradients (get_domainloss_D on probabilities, util.py:464-468) */
int srgan_mse_pair(const float* a, const float* b, long long n, float weight, float* loss, float* da, float* db,
                   void* stream);
/* generic `criterion_class(output_class, true_label)` of get_domainloss_D (util.py:464-468) on probabilities: SRGAN_CRIT_MSE
 * is srgan_mse_pair; SRGAN_CRIT_BCE is nn.BCELoss(a, b) * weight, a in [0, 1] the probabilities and b the targets, with
 * da = weight * (a - b) / max(a (1 - a), 1e-12) / n; the targets take no gradient (db must be NULL). */
int srgan_crit_pair(const float* a, const float* b, long long n, float weight, int kind, float* loss, float* da, float* db,
                    void* stream);
/* GaussianHistogram.forward (util.py:521-537) of a 1-D sample x[n] -> h[bins], and its vector-Jacobian product */
size_t srgan_soft_histogram_workspace(long long n, int bins);
int srgan_soft_histogram_fwd(const float* x, long long n, int bins, float lo, float hi, float sigma, float* h,
                             void* ws, size_t ws_bytes, void* stream);
int srgan_soft_histogram_bwd(const float* x, const float* g, long long n, int bins, float lo, float hi, float sigma,
                             float* dx, void* stream);

/* optim.Adam.step, torch 1.4 arithmetic (util_notebook.py:500-506) on flat buffers.
 * step_count is the 1-based step number t.  Writes through raw pointers (no autograd version bump).  n = 0 does nothing and
 * accepts null pointers. */
int srgan_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                    float beta2, float eps, int step_count, void* stream);

/* The same update for a whole parameter list in ONE launch.  `table` (device memory): n_tensors records of five
 * 64-bit words {p, g, m, v, numel}; all tensors must share the step count (they do: one optimiser = one list). */
int srgan_adam_multi(const void* table, int n_tensors, long long max_numel, float lr, float beta1, float beta2,
                     float eps, int step_count, void* stream);

/* The optimiser as a hipGraph-capturable op (BASELINE configs[4] "hipGraph step"; the step captured is
 * util_notebook.py:696-734): the step counter t and the hyper-parameters live in a 32-byte DEVICE record, so replaying a
 * captured train step advances t like calling optimizer.step() would.  srgan_adam_multi_dev = t += 1, bias corrections of
 * torch 1.4's Adam from the device-side t (in double), then the update of srgan_adam_multi -- two launches, no host value
 * baked into the launch.  `steps_done` seeds t (0 for a fresh optimiser; the checkpoint's count when resuming);
 * srgan_adam_state_set_lr follows lr_scheduler.ExponentialLR (util_notebook.py:501-507) between steps. */
size_t srgan_adam_state_bytes(void);
int srgan_adam_state_init(void* state, float lr, float beta1, float beta2, float eps, int steps_done, void* stream);
int srgan_adam_state_set_lr(void* state, float lr, void* stream);
int srgan_adam_multi_dev(const void* table, int n_tensors, long long max_numel, void* state, void* stream);

/* Exponential moving average of the sampling weights (G, and E whose mu feeds G), kept inside the train step.  Extension, no
 * counterpart in the reference.  A 16-byte DEVICE record {int n; int ramp; float decay; float c} holds the number of updates
 * done, so that replaying a captured step advances it.  srgan_ema_multi_dev = two launches: a tick (n += 1;
 * d_n = ramp ? min(decay, (1 + n) / (10 + n)) : decay in double, rounded to float once; c = 1 - d_n in float), then one kernel
 * over `table` (device memory): n_records records of five 64-bit words {dst, src, numel, kind, chunk0}.  kind 0:
 * dst <- dst + c * (src - dst) on fp32 (dst stays bit-identical where src == dst); kind 1: dst <- src bit for bit, numel in
 * 32-bit words (batch-norm running buffers are carried over, not averaged).  chunk0 is the index of the record's first chunk in
 * the flat list of srgan_ema_chunk()-element chunks of all records (a prefix sum of ceil(numel / chunk)); total_chunks is that
 * list's length.  decay must lie in [0, 1); n_done seeds n (0 for a fresh average, the checkpoint's count when resuming). */
size_t srgan_ema_state_bytes(void);
size_t srgan_ema_chunk(void);
int srgan_ema_state_init(void* state, float decay, int ramp, int n_done, void* stream);
int srgan_ema_state_set_decay(void* state, float decay, void* stream);
int srgan_ema_multi_dev(const void* table, int n_records, long long total_chunks, void* state, void* stream);

/* Device-side gradient guard of an optimiser: GradScaler's "found inf, skip the step" and
 * torch.nn.utils.clip_grad_norm_(norm_type=2) for a step the host never sees (a replayed hipGraph).  Extension, no counterpart
 * in the reference.  A 32-byte DEVICE record {float max_norm, norm, scale; int skip, steps, skipped, clipped, pad} holds the
 * decision of the last step and three cumulative counters; max_norm = +inf means no clipping (NaN and values <= 0 are refused),
 * srgan_grad_guard_state_init zeroes the counters, srgan_grad_guard_state_set_max_norm changes the threshold between steps.
 * srgan_grad_guard_reduce = two launches over `table` (device memory): n_records records of three 64-bit words
 * {g, numel, chunk0}, chunk0 as in srgan_ema_multi_dev for chunks of 4096 elements.  First one fp32 partial of sum g^2 per
 * chunk into `ws` (srgan_grad_guard_workspace(total_chunks) bytes; add depth 24 per chunk: 16 serial fused multiply-adds per
 * thread, an 8-level tree), then one workgroup sums the partials in double in a fixed order and writes norm = float(sqrt(S)),
 * skip = S is not finite, scale = skip ? 0 : min(1, max_norm / (norm + 1e-6f)) in fp32, steps += 1, skipped / clipped += 1.
 * No atomics: the result does not depend on the grid.  srgan_adam_multi_dev_guard = srgan_adam_multi_dev behind the record: the
 * tick runs as always (t += 1 even for a skipped step), the update stores nothing when skip is set and otherwise runs the same
 * arithmetic on g * scale (one fp32 multiply; the gradients are not written; scale = 1 leaves every result bit-identical).
 * srgan_grad_guard_state_set_counters (extension, no counterpart in the reference; resuming from a checkpoint): one
 * launch that writes the three cumulative counters between steps and nothing else -- max_norm keeps its own setter, norm / scale /
 * skip stay those of the last step; a negative count is refused (-1 with srgan_last_error(), no launch). */
size_t srgan_grad_guard_state_bytes(void);
int srgan_grad_guard_state_init(void* state, float max_norm, void* stream);
int srgan_grad_guard_state_set_max_norm(void* state, float max_norm, void* stream);
int srgan_grad_guard_state_set_counters(void* state, int steps, int skipped, int clipped, void* stream);
size_t srgan_grad_guard_workspace(long long total_chunks);
int srgan_grad_guard_reduce(const void* table, int n_records, long long total_chunks, void* ws, size_t ws_bytes, void* state,
                            void* stream);
int srgan_adam_multi_dev_guard(const void* table, int n_tensors, long long max_numel, void* adam_state, void* guard_state,
                               void* stream);

/* Spectral normalisation of convolution weights (Miyato et al., 2018; torch.nn.utils.spectral_norm with one forward per
 * optimiser step) for the discriminator.  Extension, no counterpart in the reference; fp32 in both compute modes.  A layer is
 * W[O][I][kh][kw] viewed as Wm[O][K], K = I * kh * kw.  One record of srgan_spectral_record_bytes() = sixteen 64-bit words per
 * layer: {W, W_sn, u, v, sigma, O, K, slab0, col0, elem0, ws_part, ws_t, ws_nsq, ws_y, ws_dot, 0} -- the caller fills the five
 * device pointers (fp32, 4-byte aligned; 16-byte aligned ones take the 16-byte loads) and O, K (O * K < 2^31) in a HOST copy,
 * srgan_spectral_plan checks them, fills the other words (first work item of the layer in each of the three flat work lists,
 * float offsets into the workspace) and writes the host-side plan (srgan_spectral_plan_bytes(): {int n_records, pad; long long
 * slab_items, col_items, elem_items, ws_floats}); the caller then uploads the table once.  srgan_spectral_workspace(plan): bytes
 * of the workspace (16-byte aligned) both operations take.
 * srgan_spectral_refresh, iterate = 1: n_power_iterations times {v <- Wm^T u / max(|Wm^T u|, eps); u <- Wm v / max(|Wm v|, eps)},
 * then sigma = u^T Wm v and W_sn = W / sigma, for all records: 4 launches per iteration + 1.  iterate = 0: sigma and W_sn from the
 * stored u, v (3 launches).  srgan_spectral_project: grads = n_records device pointers (0: the layer has no gradient and is left
 * alone), each the gradient G of W_sn, replaced IN PLACE by (G - <G, W_sn> u v^T) / sigma, the gradient of W with u, v, sigma held
 * constant: 2 launches.  The launch counts do not depend on the number of layers; no atomics and no workgroup waits on another,
 * every sum has a fixed order (csrc/spectral.hip), so results do not depend on the grid.  -1 with srgan_last_error() before any
 * launch: NULL table / plan / workspace, a plan of zero records, a workspace too small or misaligned, eps not > 0,
 * n_power_iterations < 1. */
size_t srgan_spectral_record_bytes(void);
size_t srgan_spectral_plan_bytes(void);
int srgan_spectral_plan(void* host_table, int n_records, void* plan);
size_t srgan_spectral_workspace(const void* plan);
int srgan_spectral_refresh(const void* table, const void* plan, int iterate, int n_power_iterations, float eps, void* ws,
                           size_t ws_bytes, void* stream);
int srgan_spectral_project(const void* table, const void* plan, const void* grads, void* ws, size_t ws_bytes, void* stream);

/* Differentiable augmentation (DiffAugment: Zhao et al., 2020) of the images the discriminator reads.  Extension, no counterpart
 * in the reference; fp32 NHWC-dense images with C = 3 in both compute modes.  Table layout: one row of 8 floats per sample,
 * [b, s, a, ty, tx, cy, cx, 0] -- brightness offset, saturation and contrast factors, then the translation and the cutout
 * centre as exact integers stored as floats; the eighth float is not read.  flags: colour 1, translation 2, cutout 4 (a group
 * that is off is not read from the table and costs no arithmetic); cut_h x cut_w is the cutout window.  Per sample, in this order:
 * x1 = x + b; x2 = (x1 - m) s + m with m the pixel's channel mean; x3 = (x2 - M) a + M with M = mean(x) + b; x4[i][j] =
 * x3[i + ty][j + tx] or 0 outside the image; y = x4 with rows [cy - cut_h / 2, cy - cut_h / 2 + cut_h) x columns [cx - cut_w / 2,
 * cx - cut_w / 2 + cut_w) zeroed.  srgan_diffaugment_fwd writes the n0 + n1 rows of y from two sources (x1 = NULL, n1 = 0 for
 * one); table row r belongs to row r of y.  srgan_diffaugment_bwd writes gx from gy and the same table: with g' = gy zeroed in
 * the window and moved back, gx[c] = a s g'[c] + a (1 - s) / 3 * sum_c g' + (1 - a) / (3 H W) * sum g'.  Two launches each with
 * colour on (per-sample partial sums into the workspace of srgan_diffaugment_workspace(n, h, w) bytes, then one gather pass),
 * one without; no atomics and a fixed summation order, so a sample's result depends neither on N nor on its position; with
 * colour off y and gx are copies or zeros bit for bit.  -1 with srgan_last_error() before any launch: C != 3, a NULL pointer
 * (the workspace only with colour on), n <= 0, an unknown flag bit, a workspace too small. */
size_t srgan_diffaugment_workspace(int n, int h, int w);
/* table: (n0 + n1) rows of 8 floats [b, s, a, ty, tx, cy, cx, 0], row r for row r of y */
int srgan_diffaugment_fwd(const float* x0, int n0, const float* x1, int n1, const float* table, float* y, int c, int h, int w,
                          int flags, int cut_h, int cut_w, void* ws, size_t ws_bytes, void* stream);
/* table: the n rows of 8 floats [b, s, a, ty, tx, cy, cx, 0] the forward of these samples read */
int srgan_diffaugment_bwd(const float* gy, const float* table, float* gx, int n, int c, int h, int w, int flags, int cut_h,
                          int cut_w, void* ws, size_t ws_bytes, void* stream);
/* Gated forms (adaptive augmentation, below): the same arguments, and slot 7 of a table row is a skip mask -- an exact float in
 * 0..7 with the bits of flags (whatever the float holds, it is clamped as the table's integers are and masked with 7: 8.0 and
 * 1e30 read 0, -1.0 reads 7, a NaN reads 0).  A group whose bit is set is not applied to that sample: sample n with mask m comes
 * out, forward and backward and on both access paths, bit for bit as the ungated entry point gives it with flags & ~m; all
 * launched groups skipped: y is a bit copy of x, gx of gy.  The partial sums of a sample whose colour bit is skipped are neither
 * written nor read.  The ungated entry points never read slot 7. */
int srgan_diffaugment_fwd_gated(const float* x0, int n0, const float* x1, int n1, const float* table, float* y, int c, int h,
                                int w, int flags, int cut_h, int cut_w, void* ws, size_t ws_bytes, void* stream);
int srgan_diffaugment_bwd_gated(const float* gy, const float* table, float* gx, int n, int c, int h, int w, int flags, int cut_h,
                                int cut_w, void* ws, size_t ws_bytes, void* stream);

/* Adaptive discriminator augmentation (Karras et al., 2020, "Training Generative Adversarial Networks with Limited Data"): the
 * probability p with which each DiffAugment group is applied to a sample, moved on the device by the overfitting heuristic
 * r = E[sign(D(real) - thr)].  Extension, no counterpart in the reference.  Record (srgan_ada_state_bytes() = 56 bytes, device
 * memory, 8-byte aligned):
 *   offset  0 float p          4 float target     8 float step      12 float p_max    16 int interval    20 int seen
 *          24 int64 n_pos     32 int64 n_neg     40 int64 n_total   48 int adjustments 52 float last_r
 * srgan_ada_state_init writes p and the settings and zeroes the counters; srgan_ada_state_set rewrites target, step, p_max,
 * interval and (set_p != 0) p and keeps the counters; srgan_ada_state_set_counters writes seen, the three counts, adjustments and
 * last_r and nothing else (resuming from a checkpoint).  One launch each, stream-ordered.
 * srgan_ada_gate: the one gate of every augmentation stage.  rows = n rows of 16 floats: slots 0..6 the stage's table row, slots
 * 8..8 + n_groups - 1 one uniform in [0, 1) per gated group, the other slots unread -- DiffAugment (n_groups = 3):
 * [b, s, a, ty, tx, cy, cx, -, u_colour, u_translation, u_cutout, ...]; the geometric stage below (n_groups = 4):
 * [fx, k, zoom, cos, sin, -, -, -, u_flip, u_rot90, u_scale, u_rotate, ...].  One launch, one thread per sample, reads p from the
 * record and writes the n rows of 8 floats the stage's gated entry points read: slots 0..6 copied bit for bit, slot 7 = the float
 * of the mask whose bit g < n_groups is set iff !(u_g < p) and whose other bits are clear (p = 0 skips every group, p = 1 none, a
 * NaN uniform skips).  n_groups is 1 to 4; rows and table 16-byte aligned, not aliased.
 * srgan_ada_observe: maps[s] = fp32 map of scale s (n_scales <= 4), per_sample[s] its elements per row (both host arrays, read
 * before the call returns), rows_first = B the real rows at the front of each map.  One launch of one workgroup: over rows [0, B)
 * of every scale n_pos += #(v > thr), n_neg += #(v < thr), n_total += #elements (a NaN counts in n_total only), seen += 1, and
 * once seen reaches interval: r = float(n_pos - n_neg) / float(n_total), p = min(max(p + sign(r - target) * step, 0), p_max) (sign
 * 0 at equality; one fp32 add, then the clamp), last_r = r, adjustments += 1, the three counts and seen back to 0.  thr: 0.5 for
 * nn.MSELoss against the targets 1 / 0, 0 for nn.BCEWithLogitsLoss.  Integer counts: exact in any order; plain stores, no atomics.
 * -1 with srgan_last_error() before any launch: a NULL pointer, n <= 0, n_groups or n_scales outside 1..4, B <= 0, a row count <= 0, a
 * setting out of range (target or thr not finite, step < 0, not 0 <= p <= p_max <= 1, interval < 1, a negative count). */
size_t srgan_ada_state_bytes(void);
int srgan_ada_state_init(void* state, float p, float target, float step, float p_max, int interval, void* stream);
int srgan_ada_state_set(void* state, float target, float step, float p_max, int interval, int set_p, float p, void* stream);
int srgan_ada_state_set_counters(void* state, int seen, long long n_pos, long long n_neg, long long n_total, int adjustments,
                                 float last_r, void* stream);
int srgan_ada_gate(const float* rows, const void* state, float* table, int n, int n_groups, void* stream);
int srgan_ada_observe(const float* const* maps, const long long* per_sample, int n_scales, int rows_first, float thr, void* state,
                      void* stream);

/* Geometric augmentation of the images D reads (the pixel-blitting and geometric groups of Karras et al., 2020): x-flip, 90-degree
 * turns, isotropic scale and arbitrary rotation as one bilinear affine warp per sample; a second stage after DiffAugment.  fp32,
 * NHWC-dense, C == 3.  table: n rows of 8 floats [fx, k, zoom, cos, sin, 0, 0, mask]; flags: flip 1, rot90 2, scale 4, rotate 8 (a
 * group that is off takes its identity value 0, 0, 1, (1, 0)).  With cen = ((h - 1) / 2, (w - 1) / 2) output pixel q reads the
 * source at s(q) = cen + R(cos, sin) Q(k) F(fx) (q - cen) / zoom, offsets in (row, col) order, F = diag(1, 1 - 2 fx), Q the turn by
 * k * 90 degrees, R = [[cos, -sin], [sin, cos]]; y[q] is the bilinear interpolation over the four neighbours, a neighbour outside the
 * image reads 0.  srgan_geom_augment_bwd is the adjoint as a gather: gx[p] = sum_q hat(s_i(q) - p_i) hat(s_j(q) - p_j) gy[q],
 * hat(t) = max(0, 1 - |t|), over the window of radius min(ceil(zoom (|cos| + |sin|)), 3) around round(cen + zoom (R Q F)^T (p - cen)),
 * row-major: no atomics, a fixed order, a sample's result depends neither on n nor on its position.  gated != 0: slot 7 of a row
 * is a skip mask, an exact float in 0..15 with the bits of flags (srgan_ada_gate with n_groups = 4 writes it); the sample comes out bit for bit
 * as the ungated form gives it with flags & ~mask.  A sample without a group left is a bit copy; any other sample goes through the
 * weighted sum, so a pure flip / rot90 row permutes VALUES (a -0.0 comes out +0.0; inf or NaN next to a read pixel, under a zero
 * weight, makes that pixel a NaN).  Whatever a row holds: zoom is
 * clamped into [0.5, 2] (non-finite reads 1), fx and k are truncated and masked into {0, 1} and {0..3} (non-finite reads 0), a
 * non-finite cos or sin makes the rotation the identity, every coordinate is clamped before it becomes an integer and every index
 * is bounds-tested: no access outside the image for any table.  One launch each.  -1 with srgan_last_error() before any launch:
 * c != 3, a NULL pointer, n, h or w <= 0, h * w > 2^29, an unknown flag bit, y aliasing x. */
int srgan_geom_augment_fwd(const float* x, const float* table, float* y, int n, int c, int h, int w, int flags, int gated, void* stream);
int srgan_geom_augment_bwd(const float* gy, const float* table, float* gx, int n, int c, int h, int w, int flags, int gated,
                           void* stream);

/* R1 gradient penalty on real samples (Mescheder et al., 2018), gamma / 2 * E_x |grad_x D(x)|^2, for the two-scale discriminator.
 * Extension, no counterpart in the reference.  The convolution passes are the ordinary entry points above (srgan_amd/r1.py drives
 * them); these are the record and the one pass in between.  Record (srgan_r1_state_bytes() = 32 bytes, device memory):
 * {float gamma, int every, float c, float penalty, float mean_sq_norm, int updates, int n, int pad}; c = gamma * every / n.
 * srgan_r1_state_init writes gamma, every, n, c and zeroes the rest; srgan_r1_state_set rewrites gamma, every, n and c between
 * steps and keeps the counters (a recorded step reads them from the record).  srgan_r1_seed: h1 = the input gradient of the first
 * scale [n, h, w, 3], h2 = that of the second scale [n, (h - 1) / 2 + 1, (w - 1) / 2 + 1, 3] (fp32 NHWC-dense); one launch
 * writes g = h1 + pool^T(h2) scaled, u0 = c * g (pool = the 3x3 / stride-2 / padding-1 average with count_include_pad = false:
 * divisors 4, 6 or 9 by position), and one fp32 partial of sum g^2 per 4096 consecutive floats of a sample into `ws`
 * (srgan_r1_workspace(n, h, w) bytes; add depth 24 per partial: 16 serial fused multiply-adds per thread, 6 butterfly levels,
 * (w0 + w1) + (w2 + w3)); 16-byte accesses when 3 h w % 4 == 0 and h1 / u0 are 16-byte aligned, else a scalar path with the same
 * owner and order per element (same bits).  srgan_r1_finalize: one workgroup sums the partials in double in a fixed order and
 * writes mean_sq_norm = S / n, penalty = gamma * every / 2 * S / n, updates += 1.  No atomics: a sample's u0 and partials depend
 * neither on n nor on its position.  -1 with srgan_last_error() before any launch: c != 3, a NULL pointer, n / h / w <= 0,
 * gamma < 0 or not finite, every < 1, a workspace too small, u0 aliasing h1 or h2.
 * srgan_r1_state_set_updates (extension, no counterpart in the reference; resuming from a checkpoint): one launch that
 * writes the count of penalised updates between steps and nothing else -- gamma, every, c and n keep srgan_r1_state_set, penalty and
 * mean_sq_norm stay those of the last finalize; a negative count is refused (-1 with srgan_last_error(), no launch). */
size_t srgan_r1_state_bytes(void);
int srgan_r1_state_init(void* state, float gamma, int every, int n, void* stream);
int srgan_r1_state_set(void* state, float gamma, int every, int n, void* stream);
int srgan_r1_state_set_updates(void* state, int updates, void* stream);
size_t srgan_r1_workspace(int n, int h, int w);
int srgan_r1_seed(const float* h1, const float* h2, const void* state, float* u0, int n, int c, int h, int w, void* ws,
                  size_t ws_bytes, void* stream);
int srgan_r1_finalize(const void* ws, size_t ws_bytes, int n, int h, int w, void* state, void* stream);

/* Balanced consistency regularisation of the discriminator (Zhang et al., 2020; on real and generated samples: Zhao et al., 2020).
 * Extension, no counterpart in the reference.  D reads 2n images, [the n it reads anyway | T of each], and is trained to give row r
 * and row r + n the same score; T is an x-flip followed by an integer translation with zeros shifted in.
 * srgan_cr_pairs_fwd: one or two fp32 NHWC-dense sources [n0, h, w, 3] and [n1, h, w, 3] (x1 NULL exactly when n1 is 0), n = n0 + n1;
 * table: n rows of 8 floats [fx, ty, tx, 0, ...]; flags: flip 1, translation 2 (a group that is off is the identity).  ONE launch
 * writes y[2n, h, w, 3]: rows [0, n) are a bit copy of the concatenated sources, row n + r is T(x_r)[i, j] = xf[i - ty, j - tx] inside
 * the image, else 0, with xf[i, j] = fx ? x[i, w - 1 - j] : x[i, j].  T copies values (no arithmetic: -0.0 and NaN payloads arrive as
 * they are); forward only.  Whatever a row holds: fx, ty, tx are truncated and clamped (fx into {0, 1}, |ty| <= h - 1, |tx| <= w - 1)
 * while still floats, a non-finite value reads 0, every index is bounds-tested: no access outside the image for any table.  16-byte
 * accesses when 3 w % 4 == 0 and x0, x1, y are 16-byte aligned, else a scalar path that gives the same bits.  -1 with
 * srgan_last_error() before any launch: c != 3, a NULL pointer (or x1 without rows, rows without x1), n0 <= 0, n1 < 0, h or w <= 0,
 * 3 h w >= 2^31, an unknown flag bit, a pointer not 4-byte aligned, y overlapping a source.
 * Record (srgan_cr_state_bytes() = 32 bytes, device memory): {float lambda_real, float lambda_fake, int every, float cr_real,
 * float cr_fake, int updates, int pad[2]}.  srgan_cr_state_init writes the weights and every and zeroes the rest; srgan_cr_state_set
 * rewrites the weights and every between steps and keeps the counters (a recorded step reads the weights from the record);
 * srgan_cr_state_set_updates writes the count of penalised updates and nothing else (resuming from a checkpoint).  One
 * launch each.  -1 before any launch: a NULL record, a weight < 0 or not finite, every < 1, a negative count.
 * srgan_d_losses_cr: srgan_d_losses_crit on maps of rows = 2 * pairs rows whose row r + pairs is the consistency partner of row r.
 * ONE launch, one workgroup, no atomics, a fixed order.  The front `pairs` rows get everything srgan_d_losses_crit computes for a map of
 * `pairs` rows (rows_first <= pairs: the split of t_first / t_rest and the rows with a class loss); the back rows carry no GAN and no
 * class loss (dz = 0 there).  With m_s(r) the mean of row r of o[s], pairs [0, pairs_first) in group 1 (lambda_real), the rest in
 * group 2 (lambda_fake), B_g the group's pair count and c_g = lambda_g * every read from the record:
 *   cr_g = (1 / S) sum_s (1 / B_g) sum_{r in g} (m_s(r) - m_s(r + pairs))^2,
 *   d_o[s][r, j] += 2 c_g / (S B_g per_row[s]) * (m_s(r) - m_s(r + pairs)) for r < pairs, and the negative of that at r + pairs.
 * vals[7] = {gan_first, class, gan_rest, total, cr_first, cr_rest, total_with_cr = total + c_1 cr_first + c_2 cr_rest}; the record's
 * cr_real / cr_fake = cr_first / cr_rest and updates += 1.  A group with c_g == 0 or no pair is taken out by a select, not a product:
 * it adds exactly 0 to total_with_cr, its back rows' d_o is exactly 0 whatever those rows hold (NaN, Inf), and its front rows' d_o is
 * the GAN gradient's bits; an empty group's cr term is 0.  With both weights 0, vals[0..3] and the front rows of d_o and dz equal bit
 * for bit what srgan_d_losses_crit gives on the `pairs`-row prefix.  The row means of a scale are staged in LDS: pairs <=
 * SRGAN_CR_MAX_PAIRS.  -1 before any launch: what srgan_d_losses_crit refuses, a NULL record, pairs outside [1, SRGAN_CR_MAX_PAIRS],
 * rows != 2 * pairs, pairs_first or rows_first outside [0, pairs], rows * per_row[s] >= 2^31. */
#define SRGAN_CR_MAX_PAIRS 1024
int srgan_cr_pairs_fwd(const float* x0, int n0, const float* x1, int n1, const float* table, float* y, int c, int h, int w, int flags,
                       void* stream);
size_t srgan_cr_state_bytes(void);
int srgan_cr_state_init(void* state, float lambda_real, float lambda_fake, int every, void* stream);
int srgan_cr_state_set(void* state, float lambda_real, float lambda_fake, int every, void* stream);
int srgan_cr_state_set_updates(void* state, int updates, void* stream);
int srgan_d_losses_cr(const float* const* o, const long long* per_row, const float* const* z, int n_scales, int rows, int rows_first,
                      int n_class, const long long* label, float t_first, float t_rest, float w_class, int gan_kind, int class_kind,
                      float* vals, float* const* d_o, float* const* dz, int pairs, int pairs_first, void* state, void* stream);

/* LeCam regularisation of the discriminator (Tseng et al., CVPR 2021, "Regularizing Generative Adversarial Networks under Limited
 * Data").  Extension, no counterpart in the reference.  One launch per discriminator update, behind srgan_d_losses_crit or
 * srgan_d_losses_cr, on the maps o[s] [rows, per_row[s]] and the d_o[s] that call wrote.  The front `pairs` rows are what D reads
 * anyway: their first rows_first rows are real, the other pairs - rows_first generated; with rows = 2 * pairs the back rows (the
 * consistency partners) and their d_o are never touched.  n1 = rows_first per_row[s], n2 = (pairs - rows_first) per_row[s].
 * Record (srgan_lc_state_bytes() = 56 bytes, device memory): {float weight, float decay, int start, int updates, float a_real[4],
 * float a_fake[4], float penalty, int applied}.  srgan_lc_state_init writes the three settings and zeroes the rest;
 * srgan_lc_state_set rewrites the three settings between steps and keeps the rest (a recorded step reads them from the record);
 * srgan_lc_state_restore writes updates and the anchors (two HOST arrays of 4 floats) and nothing else (resuming from a
 * checkpoint).  One launch each.  -1 before any launch: a NULL record or array, weight < 0 or not finite, decay outside [0, 1),
 * start < 0, updates < 0, an anchor not finite, NaN anywhere.
 * srgan_lecam: ONE launch, one workgroup, no atomics, every sum in a fixed order (csrc/lecam.hip), no fused multiply-add.
 *   means     m_R,s / m_F,s = the fp32 mean of o[s] over the real / generated elements.
 *   anchors   with n = updates and d = (n == 0 ? 0 : decay): a_R,s <- d a_R,s + (1 - d) m_R,s, likewise a_F,s.  If any of the 2S means
 *             is not finite no anchor moves and updates stays; otherwise updates += 1.  An empty group (rows_first == 0 or == pairs)
 *             has no mean: its anchor stays and its half of the term is left out.
 *   term      R = (1 / S) sum_s [ mean_real phi(o - a_F,s)^2 + mean_fake phi(a_R,s - o)^2 ] with the UPDATED anchors as constants;
 *             phi = identity (clamp 0) or max(., 0) (clamp 1, NaN kept).
 *   gradient  active = weight != 0 && n >= start.  Active: a real element's d_o += 2 weight / (S n1) phi(o - a_F,s), a generated one's
 *             d_o -= 2 weight / (S n2) phi(a_R,s - o).  Not active: d_o is neither read nor written -- a select, not a product with 0.
 *   vals[3] = {R, active ? weight R : 0, active ? *total_in + weight R : *total_in (its bits)}; the record's penalty = R, applied =
 *   active.  total_in may point into the vals of the loss call before; it must not overlap this call's vals.
 * 16-byte accesses on map s when o[s] and d_o[s] are 16-byte aligned and per_row[s] % 4 == 0, else 4-byte ones: same bits.
 * -1 with srgan_last_error() before any launch: a NULL pointer, n_scales outside [1, 4], pairs < 1, rows neither pairs nor 2 * pairs,
 * rows_first outside [0, pairs], clamp not 0 / 1, per_row[s] <= 0, rows * per_row[s] >= 2^31, a pointer not 4-byte aligned. */
size_t srgan_lc_state_bytes(void);
int srgan_lc_state_init(void* state, float weight, float decay, int start, void* stream);
int srgan_lc_state_set(void* state, float weight, float decay, int start, void* stream);
int srgan_lc_state_restore(void* state, int updates, const float* a_real, const float* a_fake, void* stream);
int srgan_lecam(const float* const* o, const long long* per_row, int n_scales, int rows, int pairs, int rows_first, int clamp,
                const float* total_in, float* vals, float* const* d_o, void* state, void* stream);

/* Mode-seeking (diversity) regularisation of the generator: restates lossModeSeeking of MSGAN (Mao et al., CVPR 2019:
 * 1 / (mean|I1 - I2| / mean|z1 - z2| + eps)) and the per-sample clamped term of DSGAN (Yang et al., ICLR 2019:
 * -mean_i min(mean|I1_i - I2_i| / mean|z1_i - z2_i|, tau)).  Extension, no counterpart in the reference.
 * i1, i2: fp32 [b, e], dense rows of e = C H W floats, 4-byte aligned (16-byte loads are used per row where both row bases allow
 * them, with the same bits either way); z1, z2: fp32 [b, d], dense.  s_i = sum |i1_i - i2_i|, t_i = sum |z1_i - z2_i|.
 * Record (srgan_ms_state_bytes() = 32 bytes, device memory): {float weight, float eps, float tau, float ms, float weighted,
 * float d_image, float d_latent, int updates}.  srgan_ms_state_init writes the three settings and zeroes the rest; srgan_ms_state_set
 * rewrites the settings between steps and keeps the rest (a recorded step reads them from the record); srgan_ms_state_restore writes
 * updates, ms, d_image, d_latent and nothing else (resuming from a checkpoint; weighted waits for the next srgan_ms_finish).  One
 * launch each.  -1 before any launch: a NULL record, weight < 0, eps <= 0, tau < 0, a value not finite, updates < 0.
 * srgan_ms_workspace(b, e): bytes of the workspace of the two passes below (the partial sums, then 2 b doubles), 0 on bad geometry.
 * srgan_ms_rows: ONE launch; ws[n * ceil(e / 4096) + c] = the fp32 sum of |i1 - i2| over floats [4096 c, 4096 c + 4096) of row n, in
 * an order that depends on e only (csrc/diversity.hip).  Forward only.
 * srgan_ms_finish: ONE launch, one workgroup, float64 throughout: s_i from the partials in ascending order, t_i over d ascending,
 * dI = sum s_i / (b e), dz = sum t_i / (b d);
 *   form 0 (msgan): ms = dz / (dI + eps dz), 0 when dz == 0; coef[i] = -weight dz / (dI + eps dz)^2 / (b e), 0 when dz == 0;
 *   form 1 (dsgan): r_i = (s_i / e) / (t_i / d); ms = -(1 / b) sum_i (t_i == 0 or r_i > tau ? tau : r_i);
 *                   coef[i] = -weight / b * (d / t_i) / e where t_i != 0 and r_i <= tau, else 0.
 * vals[2] = {weight * ms, ms}; the record takes ms, weight * ms, dI, dz and updates += 1; weight, eps, tau are READ from the record.
 * srgan_ms_grad: ONE launch; d1[i, p] = *g * coef[i] * sign(i1[i, p] - i2[i, p]), d2 = -d1, sign(0) = 0; g a device scalar; d1 or d2
 * may be NULL (nothing is written for it), not both.  No atomics anywhere; every sum has a fixed order.
 * -1 with srgan_last_error() before any launch: a NULL pointer, b, e or d <= 0, e >= 2^31 - 4096, an unknown form, a workspace too
 * small or not 8-byte aligned, a pointer not 4-byte aligned, an output of srgan_ms_grad aliasing an input or the other output. */
size_t srgan_ms_state_bytes(void);
int srgan_ms_state_init(void* state, float weight, float eps, float tau, void* stream);
int srgan_ms_state_set(void* state, float weight, float eps, float tau, void* stream);
int srgan_ms_state_restore(void* state, int updates, float ms, float d_image, float d_latent, void* stream);
size_t srgan_ms_workspace(int b, long long e);
int srgan_ms_rows(const float* i1, const float* i2, int b, long long e, void* ws, size_t ws_bytes, void* stream);
int srgan_ms_finish(const void* ws, size_t ws_bytes, const float* z1, const float* z2, int b, long long e, int d, int form,
                    void* state, float* vals, float* coef, void* stream);
int srgan_ms_grad(const float* i1, const float* i2, const float* coef, const float* g, float* d1, float* d2, int b, long long e,
                  void* stream);

/* Structural similarity (Wang et al., 2004, "Image quality assessment: from error visibility to structural similarity") as a
 * loss term with its gradient and as a metric, and PSNR.  Extension, no counterpart in the reference.  csrc/ssim.hip.
 * x, y: fp32 [n, c, h, w] stored NHWC-dense, c in 1..3, 4-byte aligned.  The window has `window` taps per axis (odd, 3..11), `taps`
 * a HOST array of window fp32 weights (srgan_ssim_taps: the Gaussian of sigma, normalised in double, rounded to fp32); they travel
 * by value in the launch packet.  Valid positions only: ho x wo = (h - window + 1) x (w - window + 1) per plane, no padding.  Per
 * position and channel, E[.] the sum over the window with the product taps: mu_x = E[x], s_x = E[x^2] - mu_x^2, s_xy = E[xy] - mu_x
 * mu_y (no clamp), SSIM = (2 mu_x mu_y + c1)(2 s_xy + c2) / ((mu_x^2 + mu_y^2 + c1)(s_x + s_y + c2)); value_i = the mean over sample
 * i's positions and channels; term = 1 - mean_i value_i.  The kernels take the moments of x - x[i, :, 0, 0], y - y[i, :, 0, 0] (one
 * pivot per plane; the definition's value, with the cancellation of E[x^2] - mu_x^2 moved to numbers of the size of the contrast).
 * Record (srgan_ssim_state_bytes() = 32 bytes, device memory): {float weight, float c1, float c2, float term, float weighted,
 * int updates, int pad[2]}.  srgan_ssim_state_init writes the three settings and zeroes the rest; srgan_ssim_state_set rewrites the
 * settings between steps and keeps the rest (a recorded step reads them from the record); srgan_ssim_state_restore writes updates
 * and the two last values and nothing else (resuming from a checkpoint).  One launch each.  -1 before any launch: a NULL record,
 * weight < 0, c1 < 0, c2 <= 0, updates < 0, a value not finite (NaN refused).
 * srgan_ssim_workspace(...): bytes of the workspace of the three launches below -- the tile partials, then 0 (no gradient), 3 (one
 * of dx / dy) or 4 (both) coefficient maps of n ho wo c floats -- or 0 on bad geometry.
 * srgan_ssim_map: ONE launch, one workgroup per (sample, tile of 8 x 32 positions): ws takes the fp32 sum of each tile's values, in
 *   a fixed order, and with want_dx / want_dy the coefficient maps.  c1, c2 are READ from the record; state may be NULL: the
 *   arguments c1, c2 count then.
 * srgan_ssim_finish: ONE launch, one workgroup, float64: values[i] (n floats), vals[2] = {weight * term, term}; the record takes
 *   term, weight * term and updates += 1; weight is READ from the record (state NULL: 1, nothing stored).
 * srgan_ssim_grad: ONE launch, one workgroup per (sample, tile of 8 x 32 input pixels): dx and / or dy (NULL: nothing is written
 *   for it; not both NULL) = the gradient of weight * term times *g (g a device scalar, NULL: 1; state NULL: weight 1), from the maps
 *   of a srgan_ssim_map call with want_dx == (dx != NULL) and want_dy == (dy != NULL) on the same workspace.
 * No atomics; every sum has a fixed order.
 * srgan_psnr: TWO launches; out[i] (n doubles) = 10 log10(data_range^2 / mse_i), +inf at mse_i == 0, mse_i the mean of (x - y)^2 over
 *   the e floats of row i: fp32 partial sums of 4096 terms, added and divided in float64.  ws of srgan_psnr_workspace(n, e) bytes.
 * -1 with srgan_last_error() before any launch: a NULL pointer, n <= 0, c outside 1..3, window even or outside 3..11, h or w below
 * window, n c h w >= 2^31 (n e for PSNR), a tap or a setting negative or not finite (NaN refused), a workspace too small or
 * misaligned (16 bytes; PSNR: 8), a pointer not 4-byte aligned, an output of srgan_ssim_grad aliasing an input or the other output. */
size_t srgan_ssim_state_bytes(void);
int srgan_ssim_state_init(void* state, float weight, float c1, float c2, void* stream);
int srgan_ssim_state_set(void* state, float weight, float c1, float c2, void* stream);
int srgan_ssim_state_restore(void* state, int updates, float term, float weighted, void* stream);
int srgan_ssim_taps(int window, double sigma, float* taps);
size_t srgan_ssim_workspace(int n, int c, int h, int w, int window, int want_dx, int want_dy);
int srgan_ssim_map(const float* x, const float* y, int n, int c, int h, int w, int window, const float* taps, const void* state,
                   float c1, float c2, int want_dx, int want_dy, void* ws, size_t ws_bytes, void* stream);
int srgan_ssim_finish(const void* ws, size_t ws_bytes, int n, int c, int h, int w, int window, void* state, float* vals,
                      float* values, void* stream);
int srgan_ssim_grad(const float* x, const float* y, int n, int c, int h, int w, int window, const float* taps, const void* ws,
                    size_t ws_bytes, const void* state, const float* g, float* dx, float* dy, void* stream);
size_t srgan_psnr_workspace(int n, long long e);
int srgan_psnr(const float* x, const float* y, int n, long long e, float data_range, double* out, void* ws, size_t ws_bytes,
               void* stream);

/* Small host -> device upload (pointer tables: <= 1 MiB, multiple of 4 bytes) carried in kernel arguments: nothing to keep
 * alive on the host after the call returns, and a captured hipGraph stores the bytes in its node instead of re-reading a host
 * address at replay (no reference counterpart; plumbing of the multi-tensor ops above). */
int srgan_upload_small(void* dst_dev, const void* src_host, size_t nbytes, void* stream);

/* ---- compute mode.  0 (default): exact fp32 products on v_mfma_f32_32x32x2_f32 (BASELINE configs[0], [1]).
 * 1: bf16 MFMA compute for configs [2]-[4]: conv operands are rounded to bf16 (nearest even) on their way into LDS and
 * multiplied on v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- torch.autocast(bfloat16) semantics for the convolutions;
 * tensors in HBM, norms, losses and Adam stay fp32; the Winograd kernels are not used.  Process-wide; packed weights made
 * under the other mode must be re-packed (srgan_amd.ops.set_compute_dtype does). */
int srgan_set_compute_mode(int mode);
int srgan_get_compute_mode(void);

/* ---- input pipeline: transforms.CenterCrop((178,178)) -> Resize((128,128)) -> RandomHorizontalFlip ->
 * ToTensor -> MinMax(True) of the training notebooks (05-train cell 9; MinMax: pyfiles/util.py:108-155) on a batch of decoded
 * uint8 RGB images src[B][Hs][Ws][3] (device).  Resize is Pillow's antialiased BILINEAR resample: the caller passes the
 * window / 22-bit fixed-point coefficient tables of its two passes (bounds[2*i] = first source index, bounds[2*i+1] = taps;
 * coeffs[i*ksize + t]), built as Pillow's precompute_coeffs / normalize_coeffs_8bpc do -- the resized bytes are bit-exact.
 * flip[b] != 0 mirrors image b; minmax / mean0 select the per-image scaling to [0,1] / [-1,1].  dst is NHWC fp32. */
size_t srgan_preprocess_workspace(int B, int crop_h, int out_h, int out_w);
int srgan_preprocess_u8(const unsigned char* src, int B, int Hs, int Ws, int top, int left, int crop_h, int crop_w,
                        int out_h, int out_w, const int* h_bounds, const int* h_coeffs, int h_ksize,
                        const int* v_bounds, const int* v_coeffs, int v_ksize, const unsigned char* flip,
                        int minmax, int mean0, float* dst, void* ws, size_t ws_bytes, void* stream);

/* ---- evaluation path (pyfiles/evaluation.py:13-110) ------------------------------------------------
 * The VGG19-bn feature extractor (evaluation.py:13-36: torchvision's vgg19_bn features + avgpool + classifier[:6]) runs its
 * 3x3 convolutions (BatchNorm folded in eval mode, bias + ReLU in the epilogue) and Linear layers on srgan_conv2d_fwd; the
 * one op it needs beyond the train step is nn.MaxPool2d(2, 2) (NHWC, C a multiple of 4; a NaN in a window comes out, as there): */
int srgan_maxpool2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
/* PRDC (evaluation.py:98-110 -> prdc.compute_prdc, prdc==0.2, Docker/requirements.txt:13), in the steps of that package:
 * compute_pairwise_distance: dist[i][j] = ||x_i - y_j||_2 for x[N][D], y[M][D] (row-major fp32);
 * get_kth_value: the k-th smallest entry of every row (1-based, k <= 16) -- with k = nearest_k + 1 on the self-distance
 *   matrix this is compute_nearest_neighbour_distances (the radii);
 * compute_prdc: out4 = {precision, recall, density, coverage} from dist[real][fake] and the two radius vectors. */
int srgan_pairwise_dist(const float* x, int N, const float* y, int M, int D, float* dist, void* stream);
int srgan_kth_smallest_rows(const float* dist, int N, int M, int k, float* out, void* stream);
size_t srgan_prdc_workspace(int N, int M);
int srgan_prdc_from_dist(const float* dist, int N, int M, const float* r_real, const float* r_fake, int nearest_k,
                         float* out4, void* ws, size_t ws_bytes, void* stream);

/* ---- set metrics beyond the reference (csrc/metrics.hip): Frechet distance and KID over feature matrices.
 * All entries enqueue on `stream` and never synchronise; a bad argument (N < 2, m < 2, m larger than a set, D < 1, a
 * workspace that is too small, a null pointer) returns -1 before any launch and writes nothing.
 * gram_f32: g[na][nb] = A B^T for row-major fp32 matrices of D columns; row r of the product is row idx_a[r] of a[rows_a][D]
 *   (idx_a = NULL: row r; an index outside [0, rows_a) reads as a row of zeros), the same for b.  Every entry is the fp32 fma
 *   chain over the features in ascending order.
 * feature_stats: mean[D] = column means of x[N][D] (float64 sums, rounded once), a[N][D] = (x - mean) / sqrt(N - 1) in fp32,
 *   *trace = sum a^2 in float64 = the trace of the unbiased covariance.
 * kid_poly3: for every subset s, rows idx_x[s][m] of x and idx_y[s][m] of y: sums[s] = {sum_{i != j} k(x_i, x_j),
 *   sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j)} with k(u, v) = (u . v / D + 1)^3, and
 *   *kid = (1 / S) sum_s [(sums[s][0] + sums[s][1]) / (m (m - 1)) - 2 sums[s][2] / m^2].
 * jacobi_sweep: one sweep of one-sided Jacobi rotations over the n vectors of w[n][L] (in place); *rotations = the number of
 *   pairs it rotated (0: the vectors are orthogonal to working precision).  nuclear_from_rows: *out = sum_i |w_i|_2 in float64,
 *   the nuclear norm of w once a sweep has rotated nothing.  Both use srgan_jacobi_workspace(n) bytes, 8-byte aligned. */
int srgan_gram_f32(const float* a, int rows_a, const int* idx_a, int na, const float* b, int rows_b, const int* idx_b, int nb,
                   int D, float* g, void* stream);
size_t srgan_feature_stats_workspace(int N, int D);
int srgan_feature_stats(const float* x, int N, int D, float* mean, float* a, double* trace, void* ws, size_t ws_bytes,
                        void* stream);
size_t srgan_kid_workspace(int num_subsets, int m);
int srgan_kid_poly3(const float* x, int n_real, const float* y, int n_fake, int D, const int* idx_x, const int* idx_y,
                    int num_subsets, int m, double* sums, double* kid, void* ws, size_t ws_bytes, void* stream);
size_t srgan_jacobi_workspace(int n);
int srgan_jacobi_sweep(float* w, int n, int L, int* rotations, void* ws, size_t ws_bytes, void* stream);
int srgan_nuclear_from_rows(const float* w, int n, int L, double* out, void* ws, size_t ws_bytes, void* stream);

/* ---- collectives of the data-parallel step (SURVEY.md 8 e) -----------------------------------------------------------
 * What replaces torch.nn.DataParallel(net, devices=[0,1,2,3]) of notebook/05-train_Style-Restricted_GAN.ipynb:404-407,446
 * (scatter the batch, replicate the module, gather the outputs, reduce the gradients on device 0): one process per GPU with
 * persistent replicas, a bucketed in-place gradient all-reduce and an all-gather of the encoder's mu rows, over RCCL (xGMI).
 * librccl.so is bound lazily at the first call (srgan_comm_available() asks without a communicator); `comm` is an opaque
 * ncclComm_t.  The calls only enqueue on `stream` (capturable into a hipGraph on a communication stream); buffers are device
 * memory owned by the caller; rendezvous -- moving the 128-byte id from rank 0 to the others -- is the caller's.
 * Return values: 0, <0 invalid argument / library unavailable, 1000 + ncclResult_t for an RCCL error. */
int srgan_comm_available(void);
int srgan_comm_unique_id(void* id128);                          /* rank 0: ncclGetUniqueId */
int srgan_comm_init(const void* id128, int nranks, int rank, void** comm);
int srgan_comm_size(void* comm, int* nranks);
int srgan_comm_destroy(void* comm);
/* gradient bucket: in-place all-reduce of `count` elements (fp32, or bf16 when `bf16` = 1), sum or average over the ranks --
 * DataParallel's reduce_add of the replicas' gradients (torch/nn/parallel/_functions.py as used by the notebook's wrapper) */
int srgan_allreduce_bucket(void* comm, void* buf, long long count, int bf16, int average, void* stream);
/* mu rows of every rank, rank-major: the gather of the replicas' encoder outputs DataParallel performs before the batch-statistics
 * losses of pyfiles/util.py:455-553 see the GLOBAL batch */
int srgan_allgather_rows(void* comm, const float* rows, float* all_rows, long long count_per_rank, void* stream);

/* ---- launch timer for bench.py's roofline leg (no reference counterpart) ---------------------
 * While enabled every implicit-GEMM / weight-gradient launch is bracketed by HIP events on its own
 * stream and tagged with its algorithmic FLOPs (2*N*Ho*Wo*O*kh*kw*I).  Collect after a device sync. */
int srgan_prof_enable(int on);
int srgan_prof_num_kernels(void);
const char* srgan_prof_kernel_name(int kid);
int srgan_prof_collect(int kid, double* total_ms, long long* launches, double* total_flops);
int srgan_prof_num_slots(void);
int srgan_prof_slot(int index, int* kid, double* ms, double* flops);

#ifdef __cplusplus
}
#endif
#endif /* SRGAN_HIP_H */
