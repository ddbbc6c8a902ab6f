/*
 * mrfp_hip.h -- C ABI of libmrfp_hip.so: the MI355X (gfx950) kernels behind the MRFP+ training
 * hot path (reference airl-iisc/MRFP: deepv3.py:152-367 and its callees).
 *
 * The reference has no native code and no FFI: its hot path is torch.nn modules calling
 * ATen/cuDNN.  Each entry point below names the reference call site (file:line) whose
 * arithmetic it replaces.  The Python side (mrfp_amd/ops.py) binds these with ctypes; see
 * INTEGRATION.md for the binding stub and the nn.Module drop-in surface.
 *
 * Conventions
 *  - plain pointers and sizes only; no torch types.  All tensor pointers are DEVICE pointers.
 *  - activations are NHWC ("channels-last"): x[b][h][w][c], dense, dtype MRFP_F32, MRFP_BF16 or MRFP_F16.
 *    Statistics, coefficients, losses and weights' master copies are always fp32.
 *  - the caller allocates every output and every workspace; nothing is allocated, freed or
 *    synchronised inside; every launch goes to `stream` (a hipStream_t passed as void*).
 *  - return 0 on success, negative on error; the message is mrfp_last_error() (thread-local).
 *  - "geometry" arguments shared by the row kernels:
 *      B, Ho, Wo, C  : logical (destination) tensor [B,Ho,Wo,C]
 *      Hs, Ws        : source tensor [B,Hs,Ws,C] when the op reads through a nearest-neighbour
 *                      resize (HRFP, reference deepv3.py:320-327); Hs==Ho, Ws==Wo otherwise
 *      tabH, tabW    : int32 device tables, tabH[oh] = source row of destination row oh
 *                      (NULL = identity).  Built on the host with ATen's float32 rule.
 */
#ifndef MRFP_HIP_H
#define MRFP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { MRFP_F32 = 0, MRFP_BF16 = 1, MRFP_F16 = 2 } mrfp_dtype;

int mrfp_version(void);
const char* mrfp_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Per-channel statistics over NHWC rows.  Replaces the reductions inside F.batch_norm
 * (reference mynn.py:19-25 Norm2d), nn.InstanceNorm2d (reference Resnet.py:176-178, 534-536),
 * feat.mean((2,3)) of NP+ (reference deepv3.py:269) and AdaptiveAvgPool2d(1) (deepv3.py:109).
 *
 * Workspace layout: float ws[B][nslab][2][C] with nslab = mrfp_stats_nslab(B, Ho);
 * ws[b][s][0][c] = partial sum, ws[b][s][1][c] = partial sum of squares (fwd), or
 * partial sum of dy' and of dy'*(x-mean) (bwd).
 * ------------------------------------------------------------------------------------------- */
int64_t mrfp_stats_nslab(int64_t B, int64_t Ho);

int mrfp_stats_fwd(const void* x, int dtype, int64_t B, int64_t Ho, int64_t Wo, int64_t C,
                   int64_t Hs, int64_t Ws, const int32_t* tabH, const int32_t* tabW,
                   float* ws, void* stream);

/* ReLU mask of the backward pass: dy' = dy * (y > 0) when y != NULL (mask from the forward output);
 * else dy' = dy * (x*fA + fS > 0) when fA/fS != NULL (mask recomputed from x with the forward apply
 * coefficients -- one tensor less to read); else dy' = dy.
 * mean, fA, fS: float [G][C] (G = B if per_image else 1); mean NULL = 0. */
int mrfp_stats_bwd(const void* dy, const void* x, const void* y, const float* mean,
                   const float* fA, const float* fS, int per_image, int dtype, int64_t B, int64_t Ho, int64_t Wo, int64_t C,
                   int64_t Hs, int64_t Ws, const int32_t* tabH, const int32_t* tabW,
                   float* ws, void* stream);
/* The same with the ReLU gate read from a SIGN MASK (1 bit per element, bit i of byte e/8 = element e of the dense [B,H,W,C]
 * tensor, written by mrfp_affine_fwd_relu_mask) instead of y: the backward of a residual block's BatchNorm -> add -> ReLU tail
 * (reference Resnet.py:202-225) needs only the sign of its output.  16-bit activations, C % 8 == 0, identity geometry. */
int mrfp_stats_bwd_mask(const void* dy, const void* x, const void* mask, const float* mean, int per_image, int dtype, int64_t B,
                        int64_t H, int64_t W, int64_t C, float* ws, void* stream);

/* BatchNorm (train): statistics over B*Ho*Wo; biased var for normalisation, unbiased for the
 * running update (momentum).  Outputs mean[C], invstd[C] and the apply coefficients
 * A[c] = w*invstd, S[c] = b - mean*A.  running_* may be NULL. */
int mrfp_bn_finalize(const float* ws, int64_t B, int64_t nslab, int64_t count, int64_t C,
                     const float* weight, const float* bias, float eps, float momentum,
                     float* running_mean, float* running_var,
                     float* mean, float* invstd, float* A, float* S, void* stream);
/* BatchNorm (eval): coefficients from the running statistics. */
int mrfp_bn_eval_coef(int64_t C, const float* weight, const float* bias, const float* running_mean,
                      const float* running_var, float eps, float* A, float* S, void* stream);
/* backward: dweight[C], dbias[C] and the input-gradient coefficients
 * dx = P*dy' + Q*x + R  (per channel). */
int mrfp_bn_bwd_finalize(const float* ws, int64_t B, int64_t nslab, int64_t count, int64_t C,
                         const float* weight, const float* mean, const float* invstd,
                         float* dweight, float* dbias, float* P, float* Q, float* R, void* stream);

/* InstanceNorm2d(affine): statistics per (b,c) over Ho*Wo, biased variance.  weight/bias may be
 * NULL (affine=False, reference instance_whitening.py:5-16).  Outputs are [B][C]. */
int mrfp_in_finalize(const float* ws, int64_t B, int64_t nslab, int64_t count, int64_t C,
                     const float* weight, const float* bias, float eps,
                     float* mean, float* invstd, float* A, float* S, void* stream);
/* dweight/dbias are accumulated over b inside (written, not added). */
int mrfp_in_bwd_finalize(const float* ws, int64_t B, int64_t nslab, int64_t count, int64_t C,
                         const float* weight, const float* mean, const float* invstd,
                         float* dweight, float* dbias, float* P, float* Q, float* R, void* stream);

/* NP+ (reference deepv3.py:268-277).  alpha, beta_noise: the two normal draws, float [B][C].
 * fwd: mu[B][C] = plane means; sigma[C] = unbiased std over the batch; scale = 1.5*sigma/max(sigma);
 *      y = A*x + S with A = alpha, S = (1 + beta_noise*scale - alpha)*mu.
 * bwd: from G[b][c] = sum_hw dy (ws from mrfp_stats_bwd with y=NULL, mean=NULL) produces the
 *      per-plane additive constant K so that dx = alpha*dy + K  (gradients flow through mu,
 *      sigma and the max exactly as autograd does for the reference expression). */
int mrfp_np_finalize(const float* ws, int64_t B, int64_t nslab, int64_t count, int64_t C,
                     const float* alpha, const float* beta_noise,
                     float* mu, float* sigma, float* A, float* S, void* stream);
int mrfp_np_bwd_finalize(const float* ws, int64_t B, int64_t nslab, int64_t count, int64_t C,
                         const float* alpha, const float* beta_noise, const float* mu,
                         const float* sigma, float* Gtmp /* scratch [B][C] */, float* K, void* stream);

/* Plane means only (AdaptiveAvgPool2d(1), reference deepv3.py:109,117): out[B][C] (dtype);
 * tmp: fp32 scratch [B][C].  Its backward (broadcast of g/(H*W)) is mrfp_affine_fwd with x = NULL. */
int mrfp_mean_finalize(const float* ws, int64_t B, int64_t nslab, int64_t count, int64_t C,
                       float* tmp, void* out, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Apply kernels.
 * fwd:  y[b,oh,ow,c] = act( x[b,tabH[oh],tabW[ow],c] * A[g,c] + S[g,c] + res[b,oh,ow,c] )
 *       g = b if coef_per_image else 0;  res may be NULL;  relu = 0/1.
 *       A == NULL means A = 1 (pure broadcast add of S), x == NULL means x = 0.
 * bwd:  dy' = dy * (y > 0) if y != NULL, else dy * (x*fA + fS > 0) if fA != NULL (see mrfp_stats_bwd)
 *       dx[b,ih,iw,c] = sum over destinations mapped to (ih,iw) of P*dy'  + n*(Q*x + R)
 *       (n = number of such destinations; invH/invW give their half-open ranges:
 *        destination rows [invH[2*ih], invH[2*ih+1]) map to source row ih; NULL = identity)
 *       dres (optional, same geometry as dy) receives dy'.
 * ------------------------------------------------------------------------------------------- */
int mrfp_affine_fwd(const void* x, const void* res, void* y, int dtype,
                    int64_t B, int64_t Ho, int64_t Wo, int64_t C, int64_t Hs, int64_t Ws,
                    const int32_t* tabH, const int32_t* tabW,
                    const float* A, const float* S, int coef_per_image, int relu, void* stream);

/* mrfp_affine_fwd (identity geometry) that also writes the per-workgroup partial sums of its STORED output, float ws[B][nslab][2][C]
 * with nslab = mrfp_stats_nslab(B, H) -- bit for bit the rows mrfp_stats_fwd(y) would produce -- for a per-image normalisation of y that
 * follows at once: the InstanceNorm behind a residual tail (reference Resnet.py:218-225) or NP+ behind an InstanceNorm
 * (deepv3.py:333-335): feed ws to mrfp_in_finalize / mrfp_np_finalize and skip their statistics pass. */
int mrfp_affine_fwd_stats(const void* x, const void* res, void* y, int dtype, int64_t B, int64_t H, int64_t W, int64_t C,
                          const float* A, const float* S, int coef_per_image, int relu, float* ws, void* stream);
int mrfp_affine_bwd(const void* dy, const void* x, const void* y, void* dx, void* dres, int dtype,
                    int64_t B, int64_t Ho, int64_t Wo, int64_t C, int64_t Hs, int64_t Ws,
                    const int32_t* invH, const int32_t* invW,
                    const float* P, const float* Q, const float* R,
                    const float* fA, const float* fS, int coef_per_image, void* stream);
/* y = relu(x*A + S + res) AND its sign mask (see mrfp_stats_bwd_mask); the matching backward apply reads the mask where
 * mrfp_affine_bwd reads y (dres = the masked gradient, for the skip connection). */
int mrfp_affine_fwd_relu_mask(const void* x, const void* res, void* y, void* mask, int dtype, int64_t B, int64_t H, int64_t W,
                              int64_t C, const float* A, const float* S, int coef_per_image, void* stream);
int mrfp_affine_bwd_mask(const void* dy, const void* x, const void* mask, void* dx, void* dres, int dtype, int64_t B, int64_t H,
                         int64_t W, int64_t C, const float* P, const float* Q, const float* R, int coef_per_image, void* stream);

/* dst[p][c0_dst + c] = src[p][c0_src + c], c < C, over npix pixels of NHWC tensors with channel pitches ld_src / ld_dst:
 * torch.cat((...), 1) of reference deepv3.py:125, 353 (one call per input) and its backward (one call per slice). */
int mrfp_copy_channels(const void* src, void* dst, int dtype, int64_t npix, int64_t C, int64_t ld_src, int64_t c0_src,
                       int64_t ld_dst, int64_t c0_dst, void* stream);

/* y = a + b, elementwise over n elements (torch.add of reference deepv3.py:330, 357). */
int mrfp_add(const void* a, const void* b, void* y, int dtype, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Bilinear resize, align_corners=True (reference mynn.py:114-119 Upsample).
 * fwd: y[B,Ho,Wo,C] = bilinear(x[B,Hi,Wi,0:C]) (+ addend[B,Ho,Wo,C] if not NULL; deepv3.py:356-357)
 * bwd: dx[B,Hi,Wi,0:C] = adjoint applied to dy[B,Ho,Wo,C]  (gather form, no atomics)
 * ld_in: channel pitch of the low-resolution tensor (>= C; the 19-class logits are kept in a
 *        32-channel padded buffer at low resolution so that the final 1x1 conv stays chunk-aligned).
 * ------------------------------------------------------------------------------------------- */
int mrfp_bilinear_fwd(const void* x, const void* addend, void* y, int dtype,
                      int64_t B, int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo, int64_t C, int64_t ld_in,
                      void* stream);
int mrfp_bilinear_bwd(const void* dy, void* dx, int dtype,
                      int64_t B, int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo, int64_t C, int64_t ld_in,
                      void* stream);
/* The same with the output (forward) / the incoming gradient (backward) being a block of C channels inside a wider NHWC tensor
 * with ld_out / ld_dy channels per pixel (y / dy point at the block's first channel): Upsample() writing straight into its
 * slot of a torch.cat(dim=1) buffer and reading its slice of that buffer's gradient (reference deepv3.py:349-353). */
int mrfp_bilinear_fwd_into(const void* x, void* y, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo,
                           int64_t C, int64_t ld_in, int64_t ld_out, void* stream);
int mrfp_bilinear_bwd_from(const void* dy, void* dx, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo,
                           int64_t C, int64_t ld_in, int64_t ld_dy, void* stream);

/* ---------------------------------------------------------------------------------------------
 * MaxPool2d(kernel 3, stride 2, padding 1) (reference Resnet.py:551, deepv3.py:315).
 * y[B,Ho,Wo,C], Ho = (H-1)/2+1; idx[B,Ho,Wo,C] (uint8) stores the window position 0..8 of the
 * first maximum.  bwd (gather form): dx[B,H,W,C] = sum of dy over windows whose arg-max is this pixel.
 * ------------------------------------------------------------------------------------------- */
int mrfp_maxpool_fwd(const void* x, void* y, uint8_t* idx, int dtype,
                     int64_t B, int64_t H, int64_t W, int64_t C, void* stream);
int mrfp_maxpool_bwd(const void* dy, const uint8_t* idx, void* dx, int dtype,
                     int64_t B, int64_t H, int64_t W, int64_t C, void* stream);

/* The stem's  norm -> ReLU -> maxpool  (reference Resnet.py:549-551, 413-421; deepv3.py:309-315) without the normalised tensor in
 * memory.  maxpool_affine_fwd pools relu(x*A + S) (A, S[C] or [B,C] as mrfp_affine_fwd; every window value is rounded to the
 * activation type before the comparison, so y and idx are those of mrfp_affine_fwd followed by mrfp_maxpool_fwd).  The two
 * backward passes of the normalisation take the POOLED gradient dy[B,Ho,Wo,C] + idx and x (the normalisation's input):
 * pool_norm_bwd_stats writes the partial sums mrfp_stats_bwd would write for the un-pooled gradient (ws: [B][mrfp_stats_nslab(B,H)]
 * [2][C] floats; ReLU gate (x*fA + fS) > 0), pool_norm_bwd_apply writes dx = P*d + Q*x + R as mrfp_affine_bwd does. */
int mrfp_maxpool_affine_fwd(const void* x, const float* A, const float* S, int coef_per_image, int relu, void* y, uint8_t* idx,
                            int dtype, int64_t B, int64_t H, int64_t W, int64_t C, void* stream);
int mrfp_pool_norm_bwd_stats(const void* dy, const uint8_t* idx, const void* x, const float* mean, const float* fA,
                             const float* fS, int coef_per_image, int relu, float* ws, int dtype,
                             int64_t B, int64_t H, int64_t W, int64_t C, void* stream);
int mrfp_pool_norm_bwd_apply(const void* dy, const uint8_t* idx, const void* x, const float* P, const float* Q, const float* R,
                             const float* fA, const float* fS, int coef_per_image, int relu, void* dx, int dtype,
                             int64_t B, int64_t H, int64_t W, int64_t C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * CrossEntropyLoss(ignore_index=255), mean over valid pixels (reference main.py:822,
 * deepv3.py:363).  logits [B,H,W,C] NHWC (dtype), target int64 [B,H,W].
 * ws: float [2*nblk] with nblk = mrfp_ce_nblocks(B*H*W).
 * fwd writes loss[0] = mean NLL, loss[1] = number of valid pixels (fp32).
 * bwd: dlogits = (softmax - onehot) * gscale[0] / nvalid  for valid pixels, 0 otherwise.
 * ------------------------------------------------------------------------------------------- */
int64_t mrfp_ce_nblocks(int64_t npix);
int mrfp_ce_fwd(const void* logits, const int64_t* target, int dtype, int64_t npix, int64_t C,
                int64_t ignore_index, float* ws, float* loss, void* stream);
int mrfp_ce_bwd(const void* logits, const int64_t* target, const float* loss, const float* gscale,
                void* dlogits, int dtype, int64_t npix, int64_t C, int64_t ignore_index, void* stream);

/* Fused bilinear upsample (align_corners) of the channel-padded low-resolution class scores P[B,Hi,Wi,ld]
 * + cross entropy at [B,H,W] (reference deepv3.py:361-365: in training only the scalar loss is needed, so the
 * full-resolution logits are never written).  ws / loss as mrfp_ce_fwd (npix = B*H*W).
 * bwd writes d(logits)[B,H,W,Cd] (Cd = C rounded up to a 16-byte chunk, pad channels zero) for mrfp_bilinear_bwd. */
int mrfp_upsample_ce_fwd(const void* P, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi,
                         int64_t H, int64_t W, int64_t C, int64_t ignore_index, float* ws, float* loss, void* stream);
int mrfp_upsample_ce_bwd(const void* P, int64_t ld, const int64_t* target, const float* loss, const float* gscale,
                         void* dlogits, int64_t Cd, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H, int64_t W,
                         int64_t C, int64_t ignore_index, void* stream);

/* Weighted / label-smoothed / per-image forms of the two losses above: the criteria a caller hands to the reference's
 * DeepV3Plus (network/deepv3.py:111 `criterion`, `criterion_aux`; main.py:822 builds the plain one).
 * weight: fp32 class weights, row b at weight + b*wstride: wstride == 0 one row [C] for all images, wstride == C one row per
 * image [B][C]; NULL = all ones.  smoothing: 0 <= eps < 1.  For a valid pixel i of image b (label t in [0,C) and != ignore_index),
 * lp = log_softmax(logits_i), w = its weight row:
 *     num_i = (1-eps) * w[t] * (-lp[t]) + (eps/C) * sum_c w[c] * (-lp[c]),      den_i = w[t]
 *     MRFP_CE_MEAN        sum_i num_i / sum_i den_i   over the batch (torch's reduction='mean'; 0/0 -> NaN)
 *     MRFP_CE_SUM         sum_i num_i
 *     MRFP_CE_IMAGE_MEAN  sum_b ( sum_{i in b} num_i / sum_{i in b} den_i )     (an all-ignored image -> NaN)
 * ws: float [2 * mrfp_ce_w_nblocks(B, HW)] (one (num, den) pair per workgroup; a workgroup stays inside one image).
 * loss: float [mrfp_ce_w_loss_floats(B, mode)]: loss[0] the loss, then the denominators the backward divides by -- loss[1] the
 * batch denominator (MEAN, SUM), loss[1 + b] the one of image b (IMAGE_MEAN).  Partial sums are reduced in double in a fixed
 * order: two runs are bit-identical.
 * bwd: dlogits_c = k * ( p_c * ((1-eps) w[t] + (eps/C) sum_j w[j]) - (1-eps) w[t] [c == t] - (eps/C) w[c] ),
 * k = gscale[0] / den (MEAN), gscale[0] (SUM), gscale[0] / den_b (IMAGE_MEAN); ignored pixels and pad channels are zeros.
 * The upsample form takes 1 <= C <= 64 and writes d(logits)[B,H,W,Cd] for mrfp_bilinear_bwd exactly as mrfp_upsample_ce_bwd. */
typedef enum { MRFP_CE_MEAN = 0, MRFP_CE_SUM = 1, MRFP_CE_IMAGE_MEAN = 2 } mrfp_ce_mode;
int64_t mrfp_ce_w_nblocks(int64_t B, int64_t HW);
int64_t mrfp_ce_w_loss_floats(int64_t B, int mode);
int mrfp_ce_w_fwd(const void* logits, const int64_t* target, int dtype, int64_t B, int64_t HW, int64_t C,
                  int64_t ignore_index, const float* weight, int64_t wstride, float smoothing, int mode, float* ws,
                  float* loss, void* stream);
int mrfp_ce_w_bwd(const void* logits, const int64_t* target, const float* loss, const float* gscale, void* dlogits,
                  int dtype, int64_t B, int64_t HW, int64_t C, int64_t ignore_index, const float* weight, int64_t wstride,
                  float smoothing, int mode, void* stream);
int mrfp_upsample_ce_w_fwd(const void* P, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi,
                           int64_t H, int64_t W, int64_t C, int64_t ignore_index, const float* weight, int64_t wstride,
                           float smoothing, int mode, float* ws, float* loss, void* stream);
int mrfp_upsample_ce_w_bwd(const void* P, int64_t ld, const int64_t* target, const float* loss, const float* gscale,
                           void* dlogits, int64_t Cd, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H, int64_t W,
                           int64_t C, int64_t ignore_index, const float* weight, int64_t wstride, float smoothing, int mode,
                           void* stream);

/* Per-image class weights from the label map, on the device (the rule of the per-image class-weighted criterion the DeepLabV3+
 * baseline was trained with; build-defined here).  n_c = number of labels equal to c in [0,C) of one image
 * (batch != 0: of all images, one output row), f_c = n_c / sum_c n_c:
 *     norm == 0:  w_c = 1 + upper_bound * (1 - f_c)        norm != 0:  w_c = 1 + upper_bound / f_c        n_c == 0:  w_c = 1
 * in double, rounded once to float.  counts_ws: int64 [B*C] scratch (cleared here); weight_out: float [B][C] ([C] if batch). */
int mrfp_label_class_weights(const int64_t* target, int64_t B, int64_t HW, int64_t C, double upper_bound, int norm,
                             int batch, int64_t* counts_ws, float* weight_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Boundary label relaxation and the joint-weighted soft-NLL loss (csrc/relax.hip).  Replaces the reference's
 * transforms/transforms.py:75-124 RelaxedBoundaryLossToTensor (config.py:56-64 BATCH_WEIGHTING, BORDER_WINDOW,
 * STRICTBORDERCLASS; utils/misc.py:51 `jointwtborder`) and the criterion that consumes its output, handed to DeepV3Plus as
 * `criterion` / `criterion_aux` (network/deepv3.py:111; its source is not in the reference tree).  Build-defined, DESIGN.md
 * section 8:
 *
 * C = number of classes, 1 <= C <= 31.  A label is a class if it lies in [0, C); every other value (255, -1, C, ...) is ignore.
 * Relaxed target R[b,y,x] (32-bit word, stored as int32) for border r, 0 <= r <= 8: the OR over the window |dy| <= r, |dx| <= r of
 * 1 << t(y+dy, x+dx), t = the label if it is a class, else C; positions outside the image give 1 << C (the reference's
 * cval = num_classes).  Bit c: class c occurs in the window; bit C: ignore / outside the image occurs.
 * strict_mask (STRICTBORDERCLASS as a bit mask): a pixel whose own label is a class in the mask gets 1 << label only.
 * The reference's scipy.ndimage.shift at integer offsets is read as a pure translation with constant fill
 * (tests/test_relaxed_cpu.py pins it); its REDUCE_BORDER_ITER branch is not built (a caller passes border / 2).
 *
 * counts (optional, int64 [B][C+1], cleared by the entry): n[b][c] = number of pixels of image b with bit c set, exact.
 * Class weights: f_c = n_c / sum_{c=0..C} n_c (the ignore plane counts in the total);
 *     norm == 0:  w_c = 1 + upper_bound * (1 - f_c)        norm != 0:  w_c = 1 + upper_bound / f_c        n_c == 0:  w_c = 1
 * in double, rounded once to float; batch != 0 pools the images into one row.  weight_out: float [B][C] ([C] if batch).
 *
 * Loss: S_i = R_i & ((1 << C) - 1); pixel i of image b is valid iff S_i is not empty; k_i = popcount(S_i), W_i = sum_{c in S_i} w_b[c]
 * (weight rows as mrfp_ce_w_fwd: wstride 0 or C, NULL = ones), lse_A(z) = log sum_{c in A} exp(z_c):
 *     l_i = (W_i / k_i) * (lse_all(z_i) - lse_{S_i}(z_i))          ( = -(W_i / k_i) log sum_{c in S_i} softmax(z_i)_c, the published
 *     L   = sum_b ( sum_{i in b, valid} l_i ) / (valid_b + 1)         per-class term log max(p_c, q_i) being log q_i on the set )
 * computed from the two log-sum-exps, each around its own maximum: a confident wrong pixel gives a finite loss and gradient.  The
 * + 1 is the published denominator: an all-ignored image contributes 0.
 * ws: float [2 * mrfp_soft_nll_nblocks(B, HW)]; loss: float [mrfp_soft_nll_loss_floats(B)]: loss[0] = L, loss[1 + b] = valid_b + 1.
 * Partials are per workgroup and reduced in double in a fixed order: two runs are bit-identical.
 * bwd: dz_c = gscale[0] * (W_i / k_i) / (valid_b + 1) * ( softmax(z_i)_c - [c in S_i] exp(z_c - lse_{S_i}) ); ignored pixels and pad
 * channels are zeros.  The upsample form works on the channel-padded low-resolution scores P[B,Hi,Wi,ld] and writes
 * d(logits)[B,H,W,Cd] (Cd = C rounded up to a 16-byte chunk) for mrfp_bilinear_bwd, exactly as mrfp_upsample_ce_w_bwd.
 * ------------------------------------------------------------------------------------------- */
int64_t mrfp_relax_nblocks(int64_t B, int64_t H, int64_t W);       /* workgroups of mrfp_relax_labels: one per 32 x 64 tile, capped */
int mrfp_relax_labels(const int64_t* target, int64_t B, int64_t H, int64_t W, int64_t C, int64_t border, int strict_mask,
                      int32_t* words, int64_t* counts, void* stream);
/* multihot: uint8 [B][C+1][HW], what the reference's transform emits; any non-zero byte is a set bit. */
int mrfp_multihot_pack(const uint8_t* multihot, int64_t B, int64_t HW, int64_t C, int32_t* words, int64_t* counts,
                       void* stream);
/* the counts of words that exist already */
int mrfp_relax_word_counts(const int32_t* words, int64_t B, int64_t HW, int64_t C, int64_t* counts, void* stream);
int mrfp_relax_class_weights(const int64_t* counts, int64_t B, int64_t C, double upper_bound, int norm, int batch,
                             float* weight_out, void* stream);
int64_t mrfp_soft_nll_nblocks(int64_t B, int64_t HW);
int64_t mrfp_soft_nll_loss_floats(int64_t B);
int mrfp_soft_nll_fwd(const void* logits, const int32_t* words, int dtype, int64_t B, int64_t HW, int64_t C,
                      const float* weight, int64_t wstride, float* ws, float* loss, void* stream);
int mrfp_soft_nll_bwd(const void* logits, const int32_t* words, const float* loss, const float* gscale, void* dlogits,
                      int dtype, int64_t B, int64_t HW, int64_t C, const float* weight, int64_t wstride, void* stream);
int mrfp_upsample_soft_nll_fwd(const void* P, int64_t ld, const int32_t* words, int dtype, int64_t B, int64_t Hi, int64_t Wi,
                               int64_t H, int64_t W, int64_t C, const float* weight, int64_t wstride, float* ws, float* loss,
                               void* stream);
int mrfp_upsample_soft_nll_bwd(const void* P, int64_t ld, const int32_t* words, const float* loss, const float* gscale,
                               void* dlogits, int64_t Cd, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H, int64_t W,
                               int64_t C, const float* weight, int64_t wstride, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Online hard example mining for the cross entropy (csrc/ohem.hip): the exact kept set of a batch on the device.  Replaces the
 * OHEM criterion (the published OhemCrossEntropy2dTensor; its source is not in the reference tree) a caller hands to DeepV3Plus as
 * `criterion` / `criterion_aux` (network/deepv3.py:111), which on the stock path materialises the full-resolution fp32 logits,
 * soft-maxes them, sorts every probability and branches on a host value.  Build-defined, DESIGN.md section 8:
 *
 * A pixel is valid iff its label t != ignore_index and 0 <= t < C.  N = valid pixels of the batch (of this rank: the selection is
 * per rank, as the published form is per replica).  p = softmax(z)[t] in fp32 for a valid pixel (a NaN is stored as 0x7fc00000).
 *     N == 0 or min_kept > N:  every valid pixel is kept                                                   (mode 0, theta = +inf)
 *     otherwise:  theta = thresh; if min_kept > 0, q = the min_kept-th smallest p of the valid pixels (from 1; NaN sorts last, as
 *                 torch.sort) and theta = q where q > thresh (a NaN q leaves thresh);  kept = valid and p <= theta: every tie at
 *                 theta is kept, a NaN p never                                        (mode 1: theta == thresh, mode 2: theta == q)
 * masked[i] = t_i where kept, ignore_index elsewhere.  The loss is CrossEntropyLoss(weight, ignore_index, 'mean') against masked
 * (mrfp_ce_* / mrfp_upsample_ce_* above; nothing kept: 0/0 = NaN, as torch); the selection is a constant for the backward.
 *
 * prob: float [B][HW], p of a valid pixel, the sentinel 2.0f for an invalid one.  The upsample form computes p from the class
 * vector rounded to the storage type, the logits mrfp_bilinear_fwd would store.  masked: int64 [B][HW].
 * ws: mrfp_ohem_ws_bytes(B, HW) bytes (cleared by the entry; -1 for a size the entries refuse).  Its first words are the state,
 * uint32: [0] N, [1] kept pixels, [2] bits of theta, [3] mode.  Nothing waits for the host or reads a device value there: the
 * regime is decided inside the kernels, so a call can be captured in a graph.  Counts are integer sums: two runs are bit-identical.
 *
 * mrfp_select_kth replaces the sort of the published form: out[0] = the k-th smallest (from 1) element of x[n], exactly, by a
 * three-level radix select (11 + 11 + 10 bits) on the bit patterns.  x: non-negative floats (unsigned order of the bits is then
 * float order; NaN last); elements equal to the sentinel 2.0f are skipped and k counts the others; k above their number: NaN.
 * ws as above.
 * ------------------------------------------------------------------------------------------- */
int64_t mrfp_ohem_ws_bytes(int64_t B, int64_t HW);
int mrfp_select_kth(const float* x, int64_t n, int64_t k, void* ws, float* out, void* stream);
int mrfp_ohem_target(const void* logits, const int64_t* target, int dtype, int64_t B, int64_t HW, int64_t C,
                     int64_t ignore_index, float thresh, int64_t min_kept, float* prob, int64_t* masked, void* ws,
                     void* stream);
int mrfp_upsample_ohem_target(const void* P, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi,
                              int64_t H, int64_t W, int64_t C, int64_t ignore_index, float thresh, int64_t min_kept,
                              float* prob, int64_t* masked, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Focal loss and the soft Dice / Jaccard region loss (csrc/loss.hip: Focal; csrc/region.hip), the criteria a caller reaches for
 * when mIoU is the metric.  Build-defined, DESIGN.md section 8.  z_i: the fp32 class vector of pixel i (dense logits, or the
 * in-kernel align-corners bilinear upsample of P), p_i = softmax(z_i); a pixel is valid iff 0 <= t_i < C and t_i != ignore_index.
 * 1 <= C <= 64 for both sources: the class vector lives in registers.
 *
 * Focal: l_i = -w[t_i] * (1 - p_{i,t})^gamma * log p_{i,t}, gamma >= 0; weight / wstride / mode / ws / loss exactly as mrfp_ce_w_*
 * (mrfp_ce_w_nblocks, mrfp_ce_w_loss_floats; den_i = w[t_i]); the argument lists are those of mrfp_ce_w_* with gamma where they
 * have smoothing.  gamma == 0 is the weighted cross entropy, bit for bit in the loss: (1 - p)^0 is the constant 1.  1 - p_t is
 * sum_{c != t} e_c / sum_c e_c, never a difference, so a pixel whose p_t rounds to 1 has loss 0 and an all-zero gradient for
 * every gamma.  bwd: dz_j = k * w[t] * (p_j - [j == t]) * ((1 - p_t)^gamma - gamma * p_t * (1 - p_t)^(gamma - 1) * log p_t), k as
 * mrfp_ce_w_bwd.  The regime of gamma is a branch inside the kernels.
 *
 * Region: over the valid pixels of a scope group (per_image == 0: the whole batch, one group; != 0: one group per image), per class
 *     I_c = sum_i p_{i,c} [t_i == c],   P_c = sum_i p_{i,c},   T_c = #{i : t_i == c}          (T_c an integer count)
 *     kind MRFP_REGION_DICE:     S_c = (2 I_c + s) / (P_c + T_c + s)
 *     kind MRFP_REGION_JACCARD:  S_c = (I_c + s) / (P_c + T_c - I_c + s)
 *     L_g = sum_{c in K} w_c (1 - S_c) / sum_{c in K} w_c,    K = {c : T_c > 0} (present_only != 0) or every c < C
 *     loss = the mean of L_g over the groups that count: those with sum_{c in K} w_c > 0 (K not empty).  None counts: 0.
 * s = smooth >= 0 (present_only == 0 needs s > 0); weight: fp32 [C], NULL = ones.  The sums are those of this process's batch.
 * ws: float [mrfp_region_ws_floats(B, HW, C)]: one partial row [3][CP] per workgroup of the (nbx, B) grid (CP = C rounded up to 8;
 * I, P as floats, T as uint32), summed by one workgroup in double in a fixed order: no floating-point atomics, two runs are
 * bit-identical.  out: float [mrfp_region_out_floats(B, C, per_image)], 8-byte aligned, rows = per_image ? B : 1:
 *     out[0] the loss; out[1] = 1 / (groups that count), 0 if none; then the coefficient table float [rows][2][CP], a_c = dL_g/dI_c
 *     and b_c = dL_g/dP_c (0 for c outside K and in a group that does not count); then the sums, double [rows][3][C] (I, P, T).
 * bwd: for a valid pixel of group g, dz_j = k * p_j * (G_j - sum_c p_c G_c), G_c = a_c [t == c] + b_c, k = gscale[0] * out[1]
 * (gscale NULL = 1); zeros for every other pixel and for pad channels; every row is stored.  The upsample forms work on the
 * channel-padded scores P[B,Hi,Wi,ld] and write d(logits)[B,H,W,Cd] for mrfp_bilinear_bwd exactly as mrfp_upsample_ce_w_bwd.
 * Nothing waits for the host: an empty K is decided inside the finalize kernel, so a call can be captured in a graph.
 * ------------------------------------------------------------------------------------------- */
int mrfp_focal_fwd(const void* logits, const int64_t* target, int dtype, int64_t B, int64_t HW, int64_t C,
                   int64_t ignore_index, const float* weight, int64_t wstride, float gamma, int mode, float* ws, float* loss,
                   void* stream);
int mrfp_focal_bwd(const void* logits, const int64_t* target, const float* loss, const float* gscale, void* dlogits,
                   int dtype, int64_t B, int64_t HW, int64_t C, int64_t ignore_index, const float* weight, int64_t wstride,
                   float gamma, int mode, void* stream);
int mrfp_upsample_focal_fwd(const void* P, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi,
                            int64_t H, int64_t W, int64_t C, int64_t ignore_index, const float* weight, int64_t wstride,
                            float gamma, int mode, float* ws, float* loss, void* stream);
int mrfp_upsample_focal_bwd(const void* P, int64_t ld, const int64_t* target, const float* loss, const float* gscale,
                            void* dlogits, int64_t Cd, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H, int64_t W,
                            int64_t C, int64_t ignore_index, const float* weight, int64_t wstride, float gamma, int mode,
                            void* stream);

typedef enum { MRFP_REGION_DICE = 0, MRFP_REGION_JACCARD = 1 } mrfp_region_kind;
int64_t mrfp_region_nblocks(int64_t B, int64_t HW);
int64_t mrfp_region_ws_floats(int64_t B, int64_t HW, int64_t C);
int64_t mrfp_region_out_floats(int64_t B, int64_t C, int per_image);
int mrfp_region_fwd(const void* logits, const int64_t* target, int dtype, int64_t B, int64_t HW, int64_t C,
                    int64_t ignore_index, const float* weight, int kind, float smooth, int present_only, int per_image,
                    float* ws, float* out, void* stream);
int mrfp_region_bwd(const void* logits, const int64_t* target, const float* out, const float* gscale, void* dlogits,
                    int dtype, int64_t B, int64_t HW, int64_t C, int64_t ignore_index, int per_image, void* stream);
int mrfp_upsample_region_fwd(const void* P, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi,
                             int64_t H, int64_t W, int64_t C, int64_t ignore_index, const float* weight, int kind, float smooth,
                             int present_only, int per_image, float* ws, float* out, void* stream);
int mrfp_upsample_region_bwd(const void* P, int64_t ld, const int64_t* target, const float* out, const float* gscale,
                             void* dlogits, int64_t Cd, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H, int64_t W,
                             int64_t C, int64_t ignore_index, int per_image, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stable segmented radix sort of (key, payload) pairs (csrc/sort.hip), the public primitive beside mrfp_select_kth: the pairs of
 * keys_in / payload_in (uint32 each, n of them, n < 2^31) sorted ascending by the low `bits` key bits (1..32; higher bits travel with
 * the key and are ignored), pairs with equal keys in their input order, independently inside each of S segments: segment s is items
 * [offsets[s], offsets[s + 1]); offsets: int64 [S + 1] on the device, non-decreasing, offsets[0] = 0 and offsets[S] = n (NULL: S = 1,
 * the whole array; zero-length segments are fine; offsets are clamped to [0, n] and every store is bounds-checked, so a wrong array
 * gives a wrong order and never a store outside the buffers).  Least-significant-digit first, 8 bits per pass, ceil(bits / 8)
 * passes of three launches (per-tile digit histogram, scan, scatter); one workgroup ranks mrfp_sort_tile_items() consecutive items
 * per pass, a scan workgroup walks the tiles of a segment mrfp_sort_scan_sweep() at a time.  No workgroup waits for another inside
 * a launch, counts are integers (two runs place every pair identically), every loop is bounded by n and S, grids are capped at 2048
 * workgroups.  The passes alternate between the outputs and ws (mrfp_sort_pairs_ws_bytes(n, S) bytes, 16-byte aligned; < 0: refused
 * size) so that the last one writes the outputs; the inputs are not written, and keys_out / payload_out may BE the inputs when the
 * number of passes is even.
 * ------------------------------------------------------------------------------------------- */
int64_t mrfp_sort_tile_items(void);
int64_t mrfp_sort_scan_sweep(void);
int64_t mrfp_sort_pairs_ws_bytes(int64_t n, int64_t S);
int mrfp_sort_pairs(const void* keys_in, const void* payload_in, void* keys_out, void* payload_out, int64_t n,
                    const int64_t* offsets, int64_t S, int bits, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018; csrc/lovasz.hip), the convex surrogate of the Jaccard index.  Not in the
 * reference tree: build-defined, DESIGN.md section 8.  Sources, z_i, p_i = softmax(z_i) (fp32) and validity as for the region loss;
 * 1 <= C <= 64, B * H * W < 2^31.  Scope: the valid pixels of this process's batch (per_image == 0) or of each image (!= 0).  Per scope
 * and class c:  f_i = [t_i == c],  e_i = |f_i - p_{i,c}|,  G = sum_i f_i.  Order the scope's pixels by e descending, ties by ascending
 * flat pixel index b * HW + p (a stable sort: the tie rule is part of the definition, it makes the gradient reproducible).  With F_i /
 * B_i the foreground / background pixels before pixel i in that order:
 *     J_i = 1 - (G - F_i - f_i) / (G + B_i + 1 - f_i),   J_i^- = 1 - (G - F_i) / (G + B_i)  (0 for the first pixel),   g_i = J_i - J_i^- >= 0
 *     loss_c = sum_i e_i g_i          (Berman's dot(errors_sorted, lovasz_grad(fg_sorted)); it does not depend on the order of ties)
 * evaluated as g_i = 1 / (G + B_i) for f_i = 1 and (G - F_i) / ((G + B_i)(G + B_i + 1)) for f_i = 0 (1 for the first pixel of a class with
 * G = 0): the same numbers without a difference of two values near 1.
 * The scope's loss is the mean of loss_c over the classes with G > 0 (all_classes == 0) or over all C (an absent class then adds the
 * largest p_c of the scope); a scope with no valid pixel has no counted class.  loss = the mean over the scopes that have a counted
 * class (the region loss's rule; the published per-image helper averages all-ignored images in as 0); none: 0.
 * bwd, g a constant: with a_i[c] = (1 - 2 f_i) g_i / (classes counted in the scope), 0 for a class that is not counted,
 *     dz_i[j] = k p_i[j] (a_i[j] - sum_c a_i[c] p_i[c]),   k = gscale[0] * out[1] (gscale NULL = 1);
 * zeros for every other pixel and for pad channels; every row is stored.  The upsample forms work on the channel-padded scores
 * P[B,Hi,Wi,ld] and write d(logits)[B,H,W,Cd] for mrfp_bilinear_bwd exactly as mrfp_upsample_region_bwd.
 *
 * fwd: classes in groups of mrfp_lovasz_group_classes() (fewer where group * B * H * W would reach 2^31).  Per group: a keys pass over
 * the source (key 0x3F800000 - bits(e), 0x3FFFFFFF for an ignored pixel: behind every valid one; payload 2 * flat index + f),
 * mrfp_sort_pairs on 30 bits with one segment per (class, scope), a three-launch integer scan of the foreground bits in sorted order
 * (per-tile count; per-segment scan, whose total is G; the third completes it inside the coefficient pass), and the coefficient
 * pass: g_i, e_i g_i into one fp32 partial per tile, (1 - 2 f_i) g_i scattered through the payload into the coefficient plane.  One
 * workgroup then sums the partials in double in a fixed order and decides class presence on the device.  No floating-point atomics,
 * no workgroup waits for another, nothing waits for the host: two runs are bit-identical and fwd + bwd can be captured in a graph.
 * ws: mrfp_lovasz_ws_bytes(B, HW, C, per_image) bytes (< 0: refused size), 16-byte aligned; bounded by the group size, not by C:
 * about 16 B * group per pixel.  out: float [mrfp_lovasz_out_floats(B, HW, C, per_image)], rows = per_image ? B : 1, CP = C rounded
 * up to 8:  out[0] the loss; out[1] = 1 / (scopes that count), 0 if none; the factor table float [rows][CP], 1 / (classes counted) for
 * a counted class of a scope that counts, else 0; then the coefficient plane float [C][B * HW], class-major, (1 - 2 f_i) g_i at every
 * valid pixel (elsewhere unwritten, and never read): the one per-pixel-per-class tensor kept for the backward.
 *
 * mrfp_lovasz_errors: the planes e as the keys pass computes them, float [C][B][H][W], 2.0 at an invalid pixel -- what a test takes the
 * device's own order from.  scores / ld / Hi / Wi: the channel-padded low-resolution scores, or with Hi == Wi == 0 dense logits
 * [B,H,W,C] (ld unused).
 * ------------------------------------------------------------------------------------------- */
int64_t mrfp_lovasz_group_classes(void);
int64_t mrfp_lovasz_ws_bytes(int64_t B, int64_t HW, int64_t C, int per_image);
int64_t mrfp_lovasz_out_floats(int64_t B, int64_t HW, int64_t C, int per_image);
int mrfp_lovasz_fwd(const void* logits, const int64_t* target, int dtype, int64_t B, int64_t HW, int64_t C,
                    int64_t ignore_index, int all_classes, int per_image, void* ws, float* out, void* stream);
int mrfp_lovasz_bwd(const void* logits, const int64_t* target, const float* out, const float* gscale, void* dlogits,
                    int dtype, int64_t B, int64_t HW, int64_t C, int64_t ignore_index, int per_image, void* stream);
int mrfp_upsample_lovasz_fwd(const void* P, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi,
                             int64_t H, int64_t W, int64_t C, int64_t ignore_index, int all_classes, int per_image, void* ws,
                             float* out, void* stream);
int mrfp_upsample_lovasz_bwd(const void* P, int64_t ld, const int64_t* target, const float* out, const float* gscale,
                             void* dlogits, int64_t Cd, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H, int64_t W,
                             int64_t C, int64_t ignore_index, int per_image, void* stream);
int mrfp_lovasz_errors(const void* scores, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi,
                       int64_t H, int64_t W, int64_t C, int64_t ignore_index, float* errors, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Two-view consistency losses (csrc/consist.hip): the criteria that compare the class scores of TWO forward passes -- the perturbed and
 * the unperturbed view of MRFP, a student and a mean teacher, a small model distilled from a large one.  Not in the reference tree:
 * build-defined, DESIGN.md section 8.  Per full-resolution pixel two fp32 class vectors: z^s, the student (it takes the gradient), and
 * z^t, the teacher.  Both views are dense logits [B,H,W,C] (mrfp_consist_*) or both are channel-padded low-resolution scores
 * P[B,Hi,Wi,ld] upsampled inside the kernel, align-corners bilinear, as every fused loss here (mrfp_upsample_consist_*); the two
 * fused views may differ in ld, Hi, Wi (a teacher with another output stride).  One dtype, one C, one (H, W).
 * 1 <= C <= mrfp_consist_max_classes() = 64: the student's class vector lives in registers, the teacher's is walked in 16-byte chunks.
 * valid: int64 [B][HW], a pixel is counted iff 0 <= valid < C (the family's rule: the ground truth can be passed as it is); NULL:
 * every pixel is counted.  N_counted = the counted pixels of this process's batch.
 * With p = softmax(z^s / T), q = softmax(z^t / T), m = (p + q) / 2, T = temperature > 0:
 *     MRFP_CONSIST_KL:    l = T^2 sum_c q_c (log q_c - log p_c);   loss = sum_counted l / N_counted.
 *                         The teacher is a constant: d loss / d z^s_j = (T / N_counted) (p_j - q_j).
 *     MRFP_CONSIST_JS:    l = T^2 (KL(p || m) / 2 + KL(q || m) / 2), the same mean.  With u_j = (log p_j - log m_j) / 2:
 *                         d loss / d z^s_j = (T / N_counted) p_j (u_j - sum_c p_c u_c), and the same with p and q exchanged for z^t.
 *                         The gradient goes to every view whose dlogits pointer is not NULL; the rows of a NULL view are not written.
 *     MRFP_CONSIST_HARD:  k = argmax_c z^t_c, the first maximum; conf = softmax(z^t)_k AT T = 1 (the temperature does not enter
 *                         this kind); the pixel is kept iff it is counted and conf >= threshold, 0 <= threshold <= 1;
 *                         l = -log softmax(z^s)_k;  loss = sum_kept l / D, D = N_kept (normalize MRFP_CONSIST_KEPT) or N_counted
 *                         (MRFP_CONSIST_VALID: the loss weighted by the confident share).  The teacher is a constant:
 *                         d loss / d z^s_j = (softmax(z^s)_j - [j == k]) / D at a kept pixel.
 * D == 0 (nothing counted, or no pixel confident): loss 0 and all-zero gradient rows, not NaN.
 * Arithmetic: fp32 per pixel in log-sum-exp form -- log p_c = z^s_c / T - lse_s, q_c log q_c as q_c (z^t_c / T - lse_t), log m_c from
 * the two log-probabilities -- so confident, disagreeing views (logits +-80) give finite losses and gradients.
 * ws: float [mrfp_consist_ws_floats(B, HW)], one partial of four words per workgroup of the (nbx, B) grid (mrfp_consist_nblocks):
 * the fp32 sum of l / T^2, N_counted and N_kept as uint32; one workgroup adds them in double / 64-bit integers in a fixed order.  No
 * floating-point atomics, nothing waits for the host: two runs are bit-identical and a call can be captured in a graph.
 * loss: float [mrfp_consist_loss_floats() = 6], 8-byte aligned: loss[0] the loss; loss[1] the backward's factor, T / D (kl, js) or 1 / D
 * (hard), 0 where D == 0; then int64 N_counted, int64 N_kept (kl, js: N_kept == N_counted).
 * bwd: every gradient is multiplied by gscale[0] (NULL = 1); a view with a dlogits pointer gets one row per pixel, zeros where the
 * pixel is not counted or not kept and in the pad channels.  dlogits_t must be NULL for kl and hard.  The upsample form writes
 * d(logits)[B,H,W,Cd], Cd = C rounded up to a 16-byte chunk, for mrfp_bilinear_bwd exactly as mrfp_upsample_region_bwd (one row
 * pitch for both views; each view's own mrfp_bilinear_bwd takes its rows down to its Hi x Wi x ld).
 * ------------------------------------------------------------------------------------------- */
typedef enum { MRFP_CONSIST_KL = 0, MRFP_CONSIST_JS = 1, MRFP_CONSIST_HARD = 2 } mrfp_consist_kind;
typedef enum { MRFP_CONSIST_KEPT = 0, MRFP_CONSIST_VALID = 1 } mrfp_consist_normalize;
int64_t mrfp_consist_max_classes(void);
int64_t mrfp_consist_nblocks(int64_t B, int64_t HW);
int64_t mrfp_consist_ws_floats(int64_t B, int64_t HW);
int64_t mrfp_consist_loss_floats(void);
int mrfp_consist_fwd(const void* logits_s, const void* logits_t, const int64_t* valid, int dtype, int64_t B, int64_t HW, int64_t C,
                     int kind, float temperature, float threshold, int normalize, float* ws, float* loss, void* stream);
int mrfp_consist_bwd(const void* logits_s, const void* logits_t, const int64_t* valid, const float* loss, const float* gscale,
                     void* dlogits_s, void* dlogits_t, int dtype, int64_t B, int64_t HW, int64_t C, int kind, float temperature,
                     float threshold, void* stream);
int mrfp_upsample_consist_fwd(const void* P_s, int64_t ld_s, int64_t Hi_s, int64_t Wi_s, const void* P_t, int64_t ld_t,
                              int64_t Hi_t, int64_t Wi_t, const int64_t* valid, int dtype, int64_t B, int64_t H, int64_t W,
                              int64_t C, int kind, float temperature, float threshold, int normalize, float* ws, float* loss,
                              void* stream);
int mrfp_upsample_consist_bwd(const void* P_s, int64_t ld_s, int64_t Hi_s, int64_t Wi_s, const void* P_t, int64_t ld_t,
                              int64_t Hi_t, int64_t Wi_t, const int64_t* valid, const float* loss, const float* gscale,
                              void* dlogits_s, void* dlogits_t, int64_t Cd, int dtype, int64_t B, int64_t H, int64_t W, int64_t C,
                              int kind, float temperature, float threshold, void* stream);

/* Eval: argmax over classes + 19x19 confusion histogram on the device (reference main.py:898-909,
 * metrics.py:122-126): hist[num_classes*gt + pred] += 1 for gt in [0,num_classes).  hist: int64
 * [C*C], accumulated (not cleared).  pred (optional, uint8 [npix]) receives the arg-max. */
int mrfp_argmax_hist(const void* logits, const int64_t* target, int dtype, int64_t npix, int64_t C,
                     int64_t* hist, uint8_t* pred, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Convolution on the matrix cores (implicit GEMM, NHWC).  Replaces every nn.Conv2d of the hot
 * path (reference Resnet.py:156-161, deepv3.py:96-112, 200-237) and its autograd backward.
 *
 * mrfp_pack_weight: OIHW fp32 master [N][C][R][S] -> forward pack wf[Npad][R][S][Cpad] and
 *   dgrad pack wd[C][R][S][Npad] (taps flipped), both in `dtype`, pad entries zero.
 * mrfp_conv_fwd:  y[B,Ho,Wo,0:N] (pitch ldy) = conv(x[B,H,W,C], wpack) + bias
 *   output position o reads source position o*stride - pad + r*dil; with sstride > 1 the tap
 *   exists only where that position is a multiple of sstride (then index = position / sstride):
 *   this is the dgrad of a strided convolution, run on dy with the wd pack.
 *   addend (optional, same shape / pitch / dtype as y) is added in the epilogue: the gradient of a skip
 *   connection is accumulated by the dgrad launch itself instead of a separate elementwise pass.
 *   C*sizeof(dtype) must be a multiple of 16 (pad the channels).
 * mrfp_conv_wgrad: dw[N][Ctrue][R][S] (fp32, OIHW) = sum over pixels of dy[.,n] * x[tap(.),c];
 *   ws: mrfp_conv_wgrad_ws_bytes(M = B*Ho*Wo, N, Q = R*S*C) bytes of scratch (split-K slabs,
 *   summed in a fixed order: bitwise reproducible).
 * mrfp_nchw_to_nhwc_pad: network input NCHW fp32 -> NHWC `dtype` with zero pad channels.
 * ------------------------------------------------------------------------------------------- */
int mrfp_pack_weight(const float* w, void* wf, void* wd, int dtype, int64_t N, int64_t C, int64_t R, int64_t S,
                     int64_t Npad, int64_t Cpad, void* stream);
/* All packs of a model in one launch (after the optimizer step rewrote the fp32 masters).  jobs: device array of
 *   struct { const float* w; void* wf; void* wd; int32_t N, C, R, S, Npad, Cpad; }   (48 bytes, both packs required)
 * prefix: device int64[njobs + 1], exclusive prefix sum of the jobs' brick counts ceil(Npad/64) * ceil(Cpad/bc), bc = 8 (64 for pointwise filters)
 * (one workgroup packs a brick of 64 output x 8 input channels x R x S -- 64 x 64 for pointwise filters -- through LDS); total = prefix[njobs].  Every job must have R*S <= 9. */
int mrfp_pack_weights_batched(const void* jobs, const int64_t* prefix, int64_t njobs, int64_t total, int dtype, void* stream);
int mrfp_conv_fwd(const void* x, const void* wpack, const float* bias, void* y, int dtype,
                  int64_t B, int64_t H, int64_t W, int64_t C, int64_t N, int64_t ldy, int64_t R, int64_t S,
                  int64_t Ho, int64_t Wo, int64_t stride, int64_t pad_h, int64_t pad_w, int64_t dil,
                  int64_t sstride, const void* addend, float* colstats, void* stream);
/* Folded inference form (mrfp_amd/inference.py): y = act(conv(x, wpack) + bias (+ addend)), act: 0 none, 1 ReLU (max(v, 0)),
 *   2 ReLU6 (min(max(v, 0), 6)).  mrfp_conv_fwd's arguments without colstats, plus `act` (23 arguments).  The kernel is the one
 *   mrfp_conv_fwd runs for the same operands without statistics; the activation is compiled into its epilogue and applied where the
 *   value is rounded to the activation type, so the result equals clamp(mrfp_conv_fwd(...)) BIT FOR BIT (rounding is monotone, 0 and 6
 *   are representable) and act = 0 is mrfp_conv_fwd itself.  act != 0 is a forward-launch option: sstride must be 1. */
int mrfp_conv_fwd_act(const void* x, const void* wpack, const float* bias, void* y, int dtype,
                      int64_t B, int64_t H, int64_t W, int64_t C, int64_t N, int64_t ldy, int64_t R, int64_t S,
                      int64_t Ho, int64_t Wo, int64_t stride, int64_t pad_h, int64_t pad_w, int64_t dil,
                      int64_t sstride, const void* addend, int act, void* stream);
/* Fold pack: an eval-mode BatchNorm behind a convolution folded into the convolution's forward pack.  With
 *   A[n] = bn_weight[n] / sqrt(running_var[n] + eps),  S[n] = bn_bias[n] - running_mean[n] * A[n]  (+ A[n] * conv_bias[n])
 * it writes wf[Npad][R][S][Cpad] = round(w * A[n]) (`dtype`; the product is taken in fp32 from the OIHW fp32 master and rounded
 * ONCE) and bias_out[Npad] = S (fp32); pad entries zero; no dgrad pack.  conv_bias, bn_weight (1) and bn_bias (0) may be NULL.
 * Everything happens on the device, without a host synchronisation (17 arguments). */
int mrfp_pack_weight_folded(const float* w, void* wf, const float* conv_bias, const float* bn_weight, const float* bn_bias,
                            const float* running_mean, const float* running_var, float eps, float* bias_out, int dtype,
                            int64_t N, int64_t C, int64_t R, int64_t S, int64_t Npad, int64_t Cpad, void* stream);
/* All fold packs of a model in one launch.  jobs: device array of
 *   struct { const float* w; void* wf; const float* conv_bias, *bn_weight, *bn_bias, *running_mean, *running_var; float* bias_out;
 *            float eps; int32_t N, C, R, S, Npad, Cpad, out_f32; }                                                  (96 bytes)
 * out_f32 = 1: wf is written as fp32 without rounding -- a depthwise weight [C][1][3][3] is the job N = Npad = C, C = Cpad = 1,
 * R = S = 3 with out_f32 = 1 (the [C][9] fp32 taps mrfp_dwconv_fwd_act reads).  prefix: device int64[njobs + 1], exclusive prefix sum
 * of the jobs' element counts Npad*R*S*Cpad + Npad; total = prefix[njobs] (6 arguments). */
int mrfp_pack_weights_folded_batched(const void* jobs, const int64_t* prefix, int64_t njobs, int64_t total, int dtype, void* stream);
/* colstats (optional): the epilogue also writes per-channel partial sums of the STORED output,
 * float [nblk][2][ldy] (sum, sum of squares per row block): the BatchNorm statistics pass over the conv output
 * disappears.  mrfp_conv_stats_layout describes that buffer for the launch with the same arguments (a statistics buffer, no
 * bias, no addend; wstats = 1: mrfp_conv_fwd_wstats, sstride = 1) -- the kernel the launch runs on (tile shape, the pointwise
 * kernels, the row-reuse and 64/128-channel 3x3 kernels), and with it the row blocks, depends on all of them.  It writes
 *   out[0] row_blocks   nblk, the row blocks the epilogue writes
 *   out[1] block_rows   rows of the [M][N] output one of them covers (block r = rows [r * rb, (r + 1) * rb)): when rb divides
 *                       Ho*Wo no block straddles an image and the blocks of image b are the per-image partial sums
 *                       nn.InstanceNorm2d needs (reference Resnet.py:176-178, 534-536: InstanceNorm after the stem convolutions) --
 *                       feed them to mrfp_in_finalize with nslab = Ho*Wo / rb.  NEGATIVE for the weight-stationary 3x3 kernel:
 *                       its rows are per image, -rb of them each.
 *   out[2] alloc_rows   rows of 2*ldy floats colstats must hold: large launches fold their row blocks into 64 groups appended
 *                       behind them
 *   out[3] final_first, out[4] final_count: the rows to hand to mrfp_bn_finalize (B = 1, nslab = final_count, count = B*Ho*Wo). */
int mrfp_conv_stats_layout(int dtype, int64_t B, int64_t H, int64_t W, int64_t C, int64_t N, int64_t ldy, int64_t R, int64_t S,
                           int64_t Ho, int64_t Wo, int64_t stride, int64_t pad_h, int64_t pad_w, int64_t dil, int64_t sstride, int wstats,
                           int64_t* out);
/* out[1] of mrfp_conv_stats_layout for mrfp_conv_fwd with ldy = N and wstats = 0 (0 on bad geometry). */
int64_t mrfp_conv_stats_block_rows(int dtype, int64_t B, int64_t H, int64_t W, int64_t C, int64_t N, int64_t R, int64_t S, int64_t Ho,
                                   int64_t Wo, int64_t stride, int64_t pad_h, int64_t pad_w, int64_t dil, int64_t sstride);
/* The K-loop gathers through 32-bit buffer-descriptor offsets, so one launch reads at most 3.75 GB of input; a larger
 * activation (BASELINE.json configs[4] at 16 images per GPU: 16 x 256 x 512 x 1024 bf16 = 4.3 GB) is walked in batch ranges
 * by mrfp_conv_fwd / mrfp_conv_wgrad themselves (one image must stay below the limit).  Returns 1 when B images of
 * image_bytes = H*W*C*sizeof(dtype) run as ONE launch -- only then are the fused per-row-block statistics available. */
int mrfp_conv_single_launch(int64_t B, int64_t image_bytes);
/* mrfp_conv_fwd whose fused statistics count output row m (pixel b, oh, ow) `rowweight[m]` times: the statistics of the
 * nearest-neighbour RESIZED output (rowweight = the pixel's multiplicity in the resize, 0..255) -- the HRFP stages
 * conv -> F.interpolate(nearest) -> BatchNorm(train) (reference deepv3.py:320-327) without a statistics pass over the
 * resized tensor.  rowweight: 4-byte aligned, B*Ho*Wo bytes + 256 readable bytes of padding.  Not for pointwise convolutions. */
int mrfp_conv_fwd_wstats(const void* x, const void* wpack, const float* bias, void* y, int dtype,
                         int64_t B, int64_t H, int64_t W, int64_t C, int64_t N, int64_t ldy, int64_t R, int64_t S,
                         int64_t Ho, int64_t Wo, int64_t stride, int64_t pad_h, int64_t pad_w, int64_t dil,
                         const uint8_t* rowweight, float* colstats, void* stream);
/* mrfp_conv_fwd with a GATED addend: y = conv(x) + (addend where its gate bit is set, else 0).  addend_mask holds one bit per
 * element of the dense [M][N] addend (bit e & 7 of byte e >> 3, e = m*N + n) -- the sign mask mrfp_affine_fwd_relu_mask wrote for
 * the residual tail whose incoming gradient `addend` is: the skip-connection gradient dy * [y > 0] (reference: autograd of
 * `out += residual; out = relu(out)`, Resnet.py:214-225) is then never materialised.  16-bit activations, N % 8 == 0, ldy == N. */
int mrfp_conv_fwd_gated(const void* x, const void* wpack, const float* bias, void* y, int dtype,
                        int64_t B, int64_t H, int64_t W, int64_t C, int64_t N, int64_t ldy, int64_t R, int64_t S,
                        int64_t Ho, int64_t Wo, int64_t stride, int64_t pad_h, int64_t pad_w, int64_t dil,
                        int64_t sstride, const void* addend, const void* addend_mask, void* stream);
/* mrfp_conv_fwd with a LOW-RANK epilogue operand: y = conv(x) + round(lr_x . lr_w^T) with lr_x [B*Ho*Wo][lr_k] and lr_w [N][lr_k], both
 * dense, in `dtype`; lr_k must be 32.  The product is one more k step in registers of the weight-stationary 3x3 kernel and the rank-32
 * tensor is never written: the input gradient of a pointwise classifier on a convolution's skip alias (mrfp_amd/conv.py: the `final2`
 * of the MRFP+ head, reference deepv3.py:355-361) rides in that convolution's dgrad, with lr_x = the score gradient and lr_w = the
 * classifier's dgrad pack wd[C][1][1][32].  The product is rounded to `dtype` before it is added, so the result equals, bit for bit,
 * mrfp_conv_fwd with the tensor a pointwise mrfp_conv_fwd(lr_x, lr_w) writes as its addend.  mrfp_conv_fwd's arguments plus the three;
 * 16-bit activations, addend and colstats must be NULL; an error (nothing launched) when mrfp_conv_lowrank_ok says 0 for the geometry. */
int mrfp_conv_fwd_lowrank(const void* x, const void* wpack, const float* bias, void* y, int dtype,
                          int64_t B, int64_t H, int64_t W, int64_t C, int64_t N, int64_t ldy, int64_t R, int64_t S,
                          int64_t Ho, int64_t Wo, int64_t stride, int64_t pad_h, int64_t pad_w, int64_t dil,
                          int64_t sstride, const void* addend, float* colstats, const void* lr_x, const void* lr_w, int64_t lr_k,
                          void* stream);
/* Host only: 1 when the launch plan sends a stride-1 launch of these operands (no bias, addend or statistics) to the kernel that takes
 * the low-rank operand, 0 otherwise (bad geometry and fp32 included).  The rule is the plan's own (mrfp_conv_fwd_lowrank asks it too). */
int mrfp_conv_lowrank_ok(int dtype, int64_t B, int64_t H, int64_t W, int64_t C, int64_t N, int64_t ldy, int64_t R, int64_t S,
                         int64_t Ho, int64_t Wo, int64_t stride, int64_t pad_h, int64_t pad_w, int64_t dil);
/* Diagnostic (no reference counterpart): in a library built with -DMRFP_CLOCK_STAMP=1 (tools/clock_stamp.py; never the product
 * build, where this returns -1) every convolution workgroup records d(s_memtime) and d(s_memrealtime) around its main loop; out
 * receives n pairs {shader cycles, 100 MHz ticks} of the LAST launch of `family` (0: conv_igemm, 1: pointwise, 2: wgrad).
 * In-kernel clock = cycles / ticks x 100 MHz (MI355X_MICROARCH.md, DVFS give-back).
 * family 3 (round 6, tools/phase_stamp.py): n pairs {cycles, samples}, eight per (workgroup, wave 0 / wave 4) of the two-group long-K
 * pointwise kernel -- the cycles that wave spent in each phase of its K loop (csrc/conv_pwk.hip: PhaseClock). */
int mrfp_debug_clock_stamps(int family, uint64_t* out, int64_t n);
int64_t mrfp_conv_wgrad_ws_bytes(int64_t M, int64_t N, int64_t Q);
int mrfp_conv_wgrad(const void* x, const void* dy, float* dw, void* ws, int dtype,
                    int64_t B, int64_t H, int64_t W, int64_t C, int64_t Ctrue, int64_t N, int64_t ldn,
                    int64_t R, int64_t S, int64_t Ho, int64_t Wo, int64_t stride, int64_t pad_h, int64_t pad_w,
                    int64_t dil, void* stream);
/* GROUPED weight gradients: `count` (<= mrfp_conv_wgrad_group_max()) problems of ONE geometry -- the repeated blocks of a ResNet
 * stage (reference network/Resnet.py:579-585 _make_layer builds blocks-1 identical Bottlenecks; autograd of Resnet.py:202-216
 * produces their weight gradients one by one) -- in ONE launch + ONE slab reduction: count x the output tiles fill the chip with
 * 2-3 K' splits per problem instead of 21-32.  xs / dys / dws: HOST arrays of `count` device pointers (x[g], dy[g] as in
 * mrfp_conv_wgrad; dws[g] = that problem's OIHW fp32 gradient); ws: mrfp_conv_wgrad_grouped_ws_bytes(M, N, Q, count) bytes.
 * Every problem's result equals a mrfp_conv_wgrad_grouped call of the same count (fixed summation order: bitwise reproducible);
 * it differs from the single launch's only in the association of the K' splits.  Each activation must fit one 3.75 GB range. */
int64_t mrfp_conv_wgrad_group_max(void);
int64_t mrfp_conv_wgrad_grouped_ws_bytes(int64_t M, int64_t N, int64_t Q, int64_t count);
/* Host only: the launch plan of mrfp_conv_wgrad (count = 1) / mrfp_conv_wgrad_grouped with the same arguments, after the same argument
 * checks (of a call that is walked in batch ranges: its first range).
 *   out[0] kernel   0 conv_wg3_kernel, 1 conv_wg1_kernel, conv_wgrad_kernel's tiles: 2 = 64 x 256, 3 = 128 x 128, 4 = 256 x 128
 *   out[1] variant  conv_wg3_kernel: strip form 0 / 1 / 2 = 64 x 1, 96 x 1, 48 x 2; the tiles: bit 0 LDS-DMA fill, bit 1 dense X rows
 *   out[2] splits   fp32 slab slots per problem (splits * count * N * Q * 4 bytes <= what the workspace queries return)
 *   out[3] klen     pixels behind one slot (K' range of a split; main chunk of the accumulator-stationary kernels)
 *   out[4] grid     workgroups */
int mrfp_conv_wgrad_plan(int dtype, int64_t B, int64_t H, int64_t W, int64_t C, int64_t N, int64_t ldn, int64_t R, int64_t S, int64_t Ho,
                         int64_t Wo, int64_t stride, int64_t pad_h, int64_t pad_w, int64_t dil, int64_t count, int64_t* out);
int mrfp_conv_wgrad_grouped(const void* const* xs, const void* const* dys, float* const* dws, int64_t count, void* ws, int dtype,
                            int64_t B, int64_t H, int64_t W, int64_t C, int64_t Ctrue, int64_t N, int64_t ldn,
                            int64_t R, int64_t S, int64_t Ho, int64_t Wo, int64_t stride, int64_t pad_h, int64_t pad_w,
                            int64_t dil, void* stream);
int mrfp_nchw_to_nhwc_pad(const float* x, void* y, int dtype, int64_t B, int64_t C, int64_t H, int64_t W,
                          int64_t Cpad, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused SGD(momentum, weight decay) over a flat fp32 arena (reference main.py:826-839, 863-864):
 *   g' = g*gscale + wd*p ; m = g' (first) | momentum*m + g' ; p -= lr*m.   n % 4 == 0.
 * ------------------------------------------------------------------------------------------- */
int mrfp_sgd_step(float* p, const float* g, float* m, int64_t n, float lr, float momentum,
                  float weight_decay, float gscale, int first, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gradient accumulation over micro-batches on the flat arenas:
 *   first != 0: acc[i] = g[i] (a bit copy; acc is not read);  otherwise acc[i] = acc[i] + g[i], one fp32 addition per element,
 *   in this operand order.  One streaming launch (16-byte loads and stores, the capped grid of mrfp_sgd_step), no atomics, no
 *   workspace; touches nothing outside [0, n).  Called on the whole arena and on contiguous sub-ranges (a data-parallel bucket):
 *   any n that is a positive multiple of 4, any 16-byte-aligned acc / g.
 * Replaces autograd's AccumulateGrad over k backward passes -- `optimizer.zero_grad()` once per k iterations in a stock loop.
 * The backward kernels here OVERWRITE their slot of the gradient arena, so the sum over a window is kept by this entry: the
 * harness calls it with (acc, g) = (accumulator, gradient arena) after each of the first k-1 passes and with the arenas in the
 * other roles after the last, which leaves the sum where mrfp_sgd_step / mrfp_grad_check / mrfp_sgd_step_checked read it.
 * The reference's loop (main.py:860-864) does not accumulate: build-defined.
 * Refused before any launch: null pointers, n <= 0, n % 4 != 0, a misaligned acc or g.
 * ------------------------------------------------------------------------------------------- */
int mrfp_grad_accumulate(float* acc, const float* g, int64_t n, int first, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Checked step: dynamic loss scale, skip on a non-finite gradient and gradient-norm clipping decided ON THE DEVICE -- the
 * semantics of torch.amp.GradScaler (unscale_ / step / update, i.e. torch._amp_update_scale_) and
 * torch.nn.utils.clip_grad_norm_ around the update rule of mrfp_sgd_step, without the host read of the overflow flag.
 * The reference trains in fp32 only (main.py:857-864), so this is build-defined.
 *
 * state: the device step state, eight 32-bit words (32 bytes), 16-byte aligned:
 *   word 0  float scale           the loss scale S; the cross-entropy backward kernels read it as their `gscale` pointer
 *   word 1  int   growth_tracker  consecutive taken steps since the scale last changed
 *   word 2  int   found_inf       1 if the last checked gradient held an inf / NaN
 *   word 3  float grad_norm       || G * gscale / S ||_2 of the last check (inf / NaN possible when found_inf)
 *   word 4  float gmul            the factor the last step applied to the raw arena gradient (0 when found_inf)
 *   word 5  int   taken           steps applied so far
 *   word 6  int   skipped         steps skipped so far
 *   word 7  reserved (0)
 *
 * mrfp_grad_check (two launches: partial sums, then a one-workgroup finalize) looks at the raw arena G = g[0..n), S = state.scale
 * and gscale (the 1/world of the data-parallel average):
 *   found_inf = any(!finite(G)), tested on the exponent bits of each element -- a large finite gradient is not an overflow;
 *   grad_norm = || G * gscale / S ||_2, accumulated in double in a fixed order (two runs are bit-identical);
 *   found_inf:  skipped += 1; dynamic: S <- S * backoff, growth_tracker <- 0;
 *   otherwise:  c = min(1, max_norm / (grad_norm + 1e-6)) (max_norm = +inf: no clipping), gmul = gscale / S * c, taken += 1;
 *               dynamic: growth_tracker += 1, and when it reaches growth_interval: S <- S * growth (kept if that is not finite),
 *               growth_tracker <- 0.
 * gmul carries the OLD scale to the step that follows; the next backward reads the new one (stream order).
 * ws: 16 * mrfp_grad_check_nblocks(n) bytes, 16-byte aligned (one {double, flag} per workgroup; no atomics).
 * Refused before any launch: null pointers, n % 4 != 0, misaligned g / ws / state, growth <= 1, backoff outside (0, 1),
 * growth_interval < 1, max_norm <= 0.
 *
 * mrfp_sgd_step_checked: found_inf set -> writes nothing (p and m stay bit for bit); else g' = g*gmul + wd*p,
 * m = momentum*m + g', p -= lr*m.  No first-step flag: m must be zero wherever no momentum exists yet (then m = g', the copy
 * torch.optim.SGD's first step makes).
 * ------------------------------------------------------------------------------------------- */
int64_t mrfp_grad_check_nblocks(int64_t n);
int mrfp_grad_check(const float* g, int64_t n, float gscale, void* ws, void* state, int dynamic, float growth,
                    float backoff, int growth_interval, float max_norm, void* stream);
int mrfp_sgd_step_checked(float* p, const float* g, float* m, int64_t n, float lr, float momentum,
                          float weight_decay, const void* state, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Weight averaging inside the step: a fourth arena e, the same size as p, holds an exponential moving average (EMA) or the
 * equal-weight mean (SWA) of the parameters after applied steps, updated while the fresh p is still in the step kernel's registers.
 * The reference keeps the last iterate only (main.py:857-869): build-defined; yardstick
 * torch.optim.swa_utils.AveragedModel over the parameters.
 *
 * The averaging rule.  t = 1-based count of APPLIED optimiser steps (a step the check skipped does not count).  An update happens
 * after step t iff t >= start and (t - start) % every == 0; its index is n = (t - start) / every.
 *   n == 0:  e = p, a bit copy of the parameters this step has just written; e is not read.
 *   n >= 1:  e = e + c * (p - e), three separately rounded fp32 operations (sub, mul, add), which is what torch's
 *            `e + c * (p - e)` gives bit for bit.  c is formed in double with IEEE operations and rounded to float once:
 *              kind 1 (swa):  c = 1 / (n + 1), the running arithmetic mean;
 *              kind 0 (ema):  d = warmup ? min(decay, (1 + n) / (10 + n)) : decay;  c = 1 - d.
 * Every thread evaluates the rule once from by-value arguments; a step that makes no update neither reads nor writes e.
 *
 * mrfp_sgd_step_avg: mrfp_sgd_step's update (p and m leave it with the same bits) followed by the rule for the step count t the
 *   host passes.  Streams 28 bytes per element against 20 when it updates with n >= 1, 24 when n == 0, 20 when it does not.
 * mrfp_sgd_step_checked_avg: mrfp_sgd_step_checked's update with t = state.taken + taken_base read on the device, after
 *   mrfp_grad_check has counted this step; found_inf set -> writes nothing, e included.  taken_base = (applied steps before this
 *   state started counting) - (state.taken at that moment): a resumed run passes what its checkpoint recorded.
 * mrfp_arena_swap: exchanges a[0..n) and b[0..n) bit for bit (NaN payloads included); the ranges must not overlap.
 * All three: one streaming launch, 16-byte loads and stores, the capped grid of mrfp_sgd_step, no LDS, no atomics, nothing outside
 *   [0, n) touched.
 * Refused before any launch: null pointers (e included), n <= 0, n % 4 != 0, a misaligned arena or state, an unknown kind, decay
 * outside (0, 1) (checked for both kinds), start < 1, every < 1, overlapping swap ranges.
 * ------------------------------------------------------------------------------------------- */
int mrfp_sgd_step_avg(float* p, const float* g, float* m, float* e, int64_t n, float lr, float momentum,
                      float weight_decay, float gscale, int first, int kind, double decay, int warmup, int start,
                      int every, int t, void* stream);
int mrfp_sgd_step_checked_avg(float* p, const float* g, float* m, float* e, int64_t n, float lr, float momentum,
                              float weight_decay, const void* state, int taken_base, int kind, double decay, int warmup,
                              int start, int every, void* stream);
int mrfp_arena_swap(float* a, float* b, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Group whitening passes (groups of 16 channels; reference network/sync_switchwhiten.py:20-26, 161-170:
 * in_data.mean(-1), bmm(in_data, in_data^T) per group; :217 bmm(wm, in_data); network/instance_whitening.py):
 *   mrfp_group_moments: M[b,g,i,j] = sum_p a[b,p,16g+i] * b[b,p,16g+j]  (fp32 [B,C/16,16,16]) and, when sum_a != NULL,
 *     sum_a[b,c] = sum_p a[b,p,c] -- one read of a and of b (a == b: second moments of the forward pass; a = dy,
 *     b = x: gradient of the whitening matrix and of the shift).  ws: mrfp_group_moments_ws_bytes() bytes of scratch
 *     (per-workgroup fp32 partials, combined in fp64 in a fixed order).
 *   mrfp_group_apply:   y[b,p,16g+i] = sum_j Wm[b,g,i,j] x[b,p,16g+j] (+ sum_j Vm[b,g,i,j] z[b,p,16g+j]) + shift[b,16g+i]
 *     (z, Vm both NULL or both given; shift optional) -- forward: the folded whitening matrix and offset; backward:
 *     dx = Wm^T dy + (dM + dM^T) x + dmean/HW in one pass.
 * a, b, x, z, y: [B,HW,C] activations (dtype); C % 16 == 0, C <= 1024.
 * ------------------------------------------------------------------------------------------- */
int64_t mrfp_group_moments_ws_bytes(int64_t B, int64_t HW, int64_t C);
int mrfp_group_moments(const void* a, const void* b, float* M, float* sum_a, void* ws, int dtype, int64_t B, int64_t HW,
                       int64_t C, void* stream);
int mrfp_group_apply(const void* x, const float* Wm, const void* z, const float* Vm, const float* shift, void* y, int dtype,
                     int64_t B, int64_t HW, int64_t C, void* stream);
/* Inverse square root of n 16x16 covariance matrices by T <= 8 Newton-Schulz steps (reference
 * sync_switchwhiten.py:206-215: P <- 1.5 P - 0.5 P^3 (S/tr S), wm = P sqrt(1/tr S)), and its backward (recomputes the
 * chain; dcov from dwm).  cov, wm, dwm, dcov: fp32 [n,16,16]. */
int mrfp_group_isqrt_fwd(const float* cov, float* wm, int64_t n, int T, void* stream);
int mrfp_group_isqrt_bwd(const float* cov, const float* dwm, float* dcov, int64_t n, int T, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fourier amplitude perturbation (north_star extension; no function of this kind exists in the
 * reference's model -- nearest arithmetic: dataloaders.py:24-79; semantics are build-defined):
 *   F = rfft2(x[b,:,:,c]); ratio = band ? ((1-lam)|F| + lam|F_partner|)/|F| : 1; y = irfft2(F*ratio)
 *   band = (min(kh,H-kh)^2 + kw^2 <= radius^2), complemented when high != 0; partner = perm[b].
 * Ws = mrfp_fourier_stored_bins(H, W, radius, high) is the number of bins along W the scratch spectra hold: W/2+1 in
 * general; floor(radius)+1 for a LOW band on the register path, where the ratio differs from 1 only in the columns
 * kw <= radius, so only those columns are transformed and y = x + irfft2(F*(ratio-1)) (same arithmetic, 2.5x less
 * HBM traffic).  S, S3: scratch spectra, float2 [B,H,Ws,C] each (mrfp_fourier_spectrum_bytes() is the upper bound);
 * ratio (optional, float [B,H,Ws,C]) is written (load_ratio = 0) or read (load_ratio = 1: the backward pass applies
 * the same detached ratio to the gradient; pass the forward call's radius and high, they fix Ws).
 * twH / twW: float2 tables exp(-2 pi i t/N), t < N, for N = H and N = W.
 * H, W of the form 2^a 3^b, <= 512, W even; C % 16 == 0.
 * ------------------------------------------------------------------------------------------- */
int64_t mrfp_fourier_spectrum_bytes(int64_t B, int64_t H, int64_t W, int64_t C);
int64_t mrfp_fourier_stored_bins(int64_t H, int64_t W, float radius, int high);
int mrfp_fourier_mix(const void* x, void* y, const int64_t* perm, void* S, void* S3, float* ratio, int load_ratio,
                     const void* twH, const void* twW, int dtype, int64_t B, int64_t H, int64_t W, int64_t C,
                     float radius, float lam, int high, void* stream);

/* Host-only: which kernel family pass `pass` of mrfp_fourier_mix(dtype, H, W, C, radius, high) runs in THIS process (the
 * launchers ask the same function, and it reads the MRFP_FFT_* A/B switches as they do), or < 0 where the call is refused.
 * pass: 0 rows forward, 1 columns (+ mix), 2 rows inverse; on the generic path 2 is the inverse column (+ mix) pass and 3 the
 * inverse row pass (the other routes have no pass 3: < 0).
 * kb, tu, nh (each may be NULL; 0 where it does not apply): of the matrix-core row passes, the 16-deep k blocks
 * ((2 Ws + 15) / 16), the pixel tiles of 16 per LDS segment (forward) or per item (inverse), and the 32-channel halves per item
 * (inverse only). */
#define MRFP_FOURIER_ROUTE_GENERIC 0  /* radix-2 / radix-3 Stockham passes, any length 2^a 3^b */
#define MRFP_FOURIER_ROUTE_TWOSTEP 1  /* two-step register transform, one channel per transform */
#define MRFP_FOURIER_ROUTE_PAIR 2     /* band-limited row pass on channel pairs */
#define MRFP_FOURIER_ROUTE_DIRECT 3   /* band-limited inverse row pass as a direct trigonometric sum */
#define MRFP_FOURIER_ROUTE_MFMA 4     /* band-limited row pass as a split-bf16 matrix product */
int mrfp_fourier_route(int dtype, int64_t H, int64_t W, int64_t C, float radius, int high, int pass, int* kb, int* tu, int* nh);

/* ---------------------------------------------------------------------------------------------
 * The training input pipeline (transform_tr), bit-exact with the PIL calls of the reference (main.py:409-419
 * transform_tr: dataloaders.py:139-150 flip, 398-435 RandomSizeAndCrop = img.resize(BICUBIC) / mask.resize(NEAREST),
 * 257-337 RandomCrop with ImageOps.expand padding, 118-136 ToTensor).  Pillow resizes 8-bit images in two separable
 * fixed-point passes: out = clip8((2^21 + sum_t in[lo + t] * coefs[o][t]) >> 22), horizontal first.
 *   mrfp_resample_u8: one pass over a uint8 [Hin,Win,C] image; bounds [out][2] = (lo, count), coefs [out][ksize] int32
 *     (host-built as Pillow builds them, mrfp_amd/input_pipeline.py); vertical = 0: Hout == Hin, flip != 0 reads the
 *     source mirrored (the reference flips before it scales); vertical = 1: Wout == Win.
 *   mrfp_input_assemble: pad (image 0 / label `ignore`) + crop + ToTensor.  img: scaled uint8 [Hs,Ws,3]; lab: ORIGINAL
 *     uint8 label map [Hl,Wl]; ytab [Hs], xtab [Ws]: Pillow's nearest-neighbour source indices of the scaled label;
 *     the scaled image sits at (pad_x, pad_y) of the padded one, the crop starts at (x1, y1); out_img float [3,Hc,Wc]
 *     (values 0..255, no /255, as dataloaders.py:128-133), out_lab int64 [Hc,Wc]; with out_u8 != NULL the image goes
 *     there as uint8 [Hc,Wc,3] instead (the blur passes run before ToTensor = mrfp_u8hwc_to_f32chw).
 *   mrfp_box_blur3_u8: one pass of ImageFilter.GaussianBlur(radius < 1) (dataloaders.py:168-177; Pillow BoxBlur.c):
 *     out = (in*ww + (left + right)*fw + 2^23) >> 24, edges replicated; GaussianBlur = 3 horizontal + 3 vertical passes;
 *     ww, fw from the radius as Pillow derives them (mrfp_amd/input_pipeline.py::_blur_weights).
 * ------------------------------------------------------------------------------------------- */
int mrfp_resample_u8(const void* src, void* dst, int64_t Hin, int64_t Win, int64_t Hout, int64_t Wout, int64_t C,
                     const int32_t* bounds, const int32_t* coefs, int ksize, int vertical, int flip, void* stream);
int mrfp_input_assemble(const void* img, const void* lab, const int32_t* ytab, const int32_t* xtab, int64_t Hs, int64_t Ws,
                        int64_t Hl, int64_t Wl, int flip, int pad_x, int pad_y, int x1, int y1, int64_t Hc, int64_t Wc, int ignore,
                        float* out_img, void* out_u8, int64_t* out_lab, void* stream);
int mrfp_box_blur3_u8(const void* src, void* dst, int64_t H, int64_t W, int64_t C, int64_t ww, int64_t fw, int vertical,
                      void* stream);
int mrfp_u8hwc_to_f32chw(const void* src, float* dst, int64_t H, int64_t W, void* stream);
/* One ColorJitter step on a uint8 [npix,3] image (dataloaders.py:491-660; Pillow ImageEnhance = Image.blend with a degenerate
 * image, Convert.c rgb2hsv / hsv2rgb): op 0 brightness, 1 contrast (needs ws: 16 bytes, the L mean is reduced on the device),
 * 2 saturation, 3 hue (shift = uint8(hue_factor * 255), factor unused).  Byte-exact with PIL. */
int mrfp_jitter_u8(const void* src, void* dst, int64_t npix, int op, float factor, int shift, void* ws, void* stream);
/* RandomRotate (dataloaders.py:153-165: img.rotate(angle, BILINEAR), mask.rotate(angle, NEAREST)) for an image / label pair in
 * one launch, byte-exact with Pillow's affine transform (Geometry.c).  img uint8 [H,W,3], lab uint8 [H,W] -> out_img, out_lab of the
 * same shapes (no aliasing).  mode 0: the affine path with the matrix (m0..m5) that Image.rotate builds (host side:
 * mrfp_amd/input_pipeline.py::rotate_plan): image by ImagingGenericTransform (double, bilinear, result truncated), label by
 * affine_fixed (16.16 fixed point); pixels that map outside are 0 in both (the reference passes no fillcolor).  Refused when a
 * corner of the image maps to 32768 or beyond (Pillow leaves the fixed-point path there; its double fallback is not built).
 * mode 1 copy, 2 ROTATE_90, 3 ROTATE_180, 4 ROTATE_270: the exact transposes Image.rotate dispatches to (2 and 4: H == W; the
 * matrix is ignored).  flip != 0 reads the source mirrored: RandomHorizontalFlip comes before RandomRotate. */
int mrfp_affine_u8(const void* img, const void* lab, void* out_img, void* out_lab, int64_t H, int64_t W, int mode, int flip,
                   double m0, double m1, double m2, double m3, double m4, double m5, void* stream);
/* Normalize (dataloaders.py:95-115) fused into ToTensor (:118-136): src uint8 [H,W,3] -> dst float32 [3,H,W],
 * v = float32(u8) / float32(255); v = float32(double(v) - mean[c]); v = float32(double(v) / std[c]) -- the precisions numpy
 * evaluates `img /= 255.0; img -= mean; img /= std` in for a float32 array and tuples of Python floats.  Bit-equal to numpy. */
int mrfp_u8hwc_to_f32chw_norm(const void* src, float* dst, int64_t H, int64_t W, double mean0, double mean1, double mean2,
                              double std0, double std1, double std2, void* stream);
/* The evaluation input path: label encoding and Mapillary's validation transform.
 *   mrfp_label_lut_u8: dst[i] = lut[src[i]] over n >= 0 bytes (n == 0 launches nothing); lut: 256 bytes on the device.  Replaces
 *     the per-class-id masked numpy passes over the label map of main.py:106-112 (encode_segmap, called at :96, :188, :290,
 *     :383), :561-563 (Synthia) and :742-745 (Mapillary): the table is those passes replayed on arange(256)
 *     (mrfp_amd/input_pipeline.py::LabelEncoder).  dst == src is allowed, any other overlap is refused; src and dst need no
 *     alignment (bytes in front of the first 16-byte boundary and behind the last go one by one; pointers that differ modulo
 *     16 take a byte path).
 *   mrfp_label_encode_i64: dst_i64[i] = (int64)lut[src_u8[i]], lut == NULL: identity.  The label half of a ToTensor-only
 *     validation sample (main.py:134-144 and the transform_val of every class but Mapillary; dataloaders.py:118-136 ToTensor)
 *     with the encoding in the same pass.  src_u8 needs no alignment, dst_i64 that of an int64.
 *   mrfp_eval_assemble: the assemble step of main.py:775-783 (dataloaders.py:354-394 CenterCropPad, :118-136 ToTensor).
 *     Operands as mrfp_input_assemble (no flip, no uint8 output), except: the crop origin (x1, y1) may be negative and the crop
 *     may leave the padded image -- such pixels are 0 in the image and 0 in the label, as Image.crop gives; pixels of the
 *     ImageOps.expand border take the label `pad_label` (0..255; the image is 0 there); lut != NULL: 256 bytes, applied to
 *     the label bytes as they are read (pad_label and the zeros are not looked up: the reference encodes before it pads). */
int mrfp_label_lut_u8(const void* src, void* dst, int64_t n, const void* lut, void* stream);
int mrfp_label_encode_i64(const void* src_u8, const void* lut, int64_t* dst_i64, int64_t n, void* stream);
int mrfp_eval_assemble(const void* img, const void* lab, const int32_t* ytab, const int32_t* xtab, int64_t Hs, int64_t Ws,
                       int64_t Hl, int64_t Wl, int pad_x, int pad_y, int x1, int y1, int64_t Hc, int64_t Wc, int pad_label,
                       const void* lut, float* out_img, int64_t* out_lab, void* stream);
/* Class-uniform sampling, the producer half (reference config.py:53-64 CLASS_UNIFORM_PCT; the published form loops
 * `for tile: for class: scipy.ndimage.center_of_mass` over label PNGs on the host -- its source is not in the reference tree, so the
 * rule below is the definition).  lab: uint8 [B,H,W] on the device, any alignment.
 *   v = table ? table[lab] : lab (table: 256 bytes on the device, the id -> train id step); a pixel belongs to class c iff v == c and
 *   c < C (255 and ids >= C belong to nothing).  Tiles are tile x tile with origin (tx * tile, ty * tile).  partial == 0: only whole
 *   tiles, H / tile by W / tile of them -- the ragged right and bottom strips are never read (the published behaviour); partial != 0:
 *   ceil tiles, the ragged ones count (this build's extension).  mrfp_tile_count(size, tile, partial) is that count along one axis
 *   (host only; -1 for tile < 1 or size < 0).
 *   sums int64 [B][nty][ntx][C][3] = n, sum(x - x0), sum(y - y0) over the class's pixels in the tile; cent int32 [B][nty][ntx][C][2] =
 *   cx, cy in image coordinates, cx = x0 + floor(sum(x - x0) / n), cy likewise -- int(center_of_mass(patch == c)) + offset of the
 *   published form -- and -1, -1 where n == 0.  Both are written in full: the entry clears what it accumulates into.
 * Three launches (clear, accumulate, divide), integers only (LDS counters, then 64-bit integer atomic adds, which commute: two runs
 * give the same bits), no host wait.  Refused on the host, by name: C outside 1..256, tile outside 1..65536, H or W >= 2^31,
 * B * nty * ntx * C >= 2^31, no tile (partial == 0 and H < tile or W < tile). */
int64_t mrfp_tile_count(int64_t size, int64_t tile, int partial);
int mrfp_tile_class_sums(const uint8_t* lab, const uint8_t* table, int64_t B, int64_t H, int64_t W, int64_t C, int64_t tile,
                         int partial, int64_t* sums, int32_t* cent, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Frequency filters of the input pipeline (reference dataloaders.py:24-45 HPF, 59-79 LPF, 47-57 PHOT: np.fft.fftn over the
 * (H,W,3) image), on the ToTensor layout: x, y float32 [B,3,H,W] (y may be x).  Signed frequencies as the reference's fftshift
 * gives them: f = i - n//2, f in [-(n//2), n-1-n//2].  twH / twW: float2 tables exp(-2 pi i t/N), t < N, N = H and N = W
 * (built in double on the host).  ws: mrfp_band_filter_ws_bytes / mrfp_phot_ws_bytes bytes (-1: arguments not supported).
 *   mrfp_band_filter: per channel plane low = Re(IDFT2(F * band)); high != 0 (HPF): band = fy^2 + fx^2 <= radius^2, y = x - low;
 *     high == 0 (LPF): band = fy^2 + fx^2 < radius^2, y = low.  A band-limited DFT (no full transform), any H, W < 65536,
 *     0 <= radius < 33; no atomics: bitwise reproducible.
 *   mrfp_phot: y = Re(ifftn(F / |F|)) * 5 * 255 over the 3-D spectrum (channel axis included); a zero bin gives NaN as numpy
 *     does (a grey image: all NaN).  H and W of the form 2^a 3^b 5^c, each <= 4096; other lengths fail naming the length.
 * ------------------------------------------------------------------------------------------- */
int64_t mrfp_band_filter_ws_bytes(int64_t B, int64_t H, int64_t W, float radius);
int mrfp_band_filter(const float* x, float* y, void* ws, const void* twH, const void* twW, int64_t B, int64_t H, int64_t W,
                     float radius, int high, void* stream);
int64_t mrfp_phot_ws_bytes(int64_t B, int64_t H, int64_t W);
int mrfp_phot(const float* x, float* y, void* ws, const void* twH, const void* twW, int64_t B, int64_t H, int64_t W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Whitening-loss setup (host-side, no kernel; csrc/hostmath.hip).
 *   mrfp_kmeans1d: globally optimal k-means of n doubles into k clusters -- what `kmeans1d.cluster(var_flatten,
 *     self.clusters)` does at reference network/cov_settings.py:57 (kmeans1d is an un-vendored PyPI dependency; its published
 *     dynamic programme over the sorted values is restated).  labels [n] int32 in input order, clusters numbered by
 *     ascending centroid; centroids [k] (k is clamped to n).  Host pointers.
 * ------------------------------------------------------------------------------------------- */
int mrfp_kmeans1d(const double* x, int64_t n, int k, int32_t* labels, double* centroids);

/* ---------------------------------------------------------------------------------------------
 * Depthwise 3x3 convolution, groups == C_in == C_out (reference network/Mobilenet.py ConvBNReLU with groups = hidden_dim,
 * the dw layer of every InvertedResidual; csrc/conv_dw.hip).  padding = dilation (any dilation >= 1), stride 1 or 2:
 * Ho = (H - 1) / stride + 1.  x, y, dx, dy: NHWC with channel pitch Cp (C rounded up to a 16-byte chunk); pad channels
 * c >= C are written as zero.  w: the fp32 OIHW master weight [C][1][3][3]; bias: fp32 [C] or NULL.  Accumulation in fp32.
 *   fwd:   y = dwconv(x, w) (+ bias).  ws (optional): BatchNorm partial statistics of the STORED y, float ws[B][nslab][2][Cp]
 *          with nslab = mrfp_dwconv_nslab(dtype, B, Ho, Cp) -- the layout mrfp_bn_finalize reads (B*nslab rows).  Summed in a
 *          fixed order: the rows are bitwise reproducible.
 *   dgrad: dx[B,H,W,Cp] (gather form: each dx pixel collects the taps that read it; no atomics).
 *   wgrad: dw[C][3][3] fp32 (written, not added), through per-workgroup slabs summed in a fixed order; ws holds
 *          mrfp_dwconv_wgrad_ws_bytes(dtype, B, Ho, Cp) bytes.
 * ------------------------------------------------------------------------------------------- */
int64_t mrfp_dwconv_nslab(int dtype, int64_t B, int64_t Ho, int64_t Cp);
int64_t mrfp_dwconv_wgrad_ws_bytes(int dtype, int64_t B, int64_t Ho, int64_t Cp);
int mrfp_dwconv_fwd(const void* x, const float* w, const float* bias, void* y, int dtype, int64_t B, int64_t H, int64_t W, int64_t Cp,
                    int64_t C, int64_t Ho, int64_t Wo, int64_t stride, int64_t dil, float* ws, void* stream);
/* folded inference form: y = act(dwconv(x, w) + bias), act as in mrfp_conv_fwd_act; mrfp_dwconv_fwd's arguments without ws, plus
 * `act` (16 arguments).  Equals clamp(mrfp_dwconv_fwd(...)) bit for bit; act = 0 is mrfp_dwconv_fwd without statistics. */
int mrfp_dwconv_fwd_act(const void* x, const float* w, const float* bias, void* y, int dtype, int64_t B, int64_t H, int64_t W, int64_t Cp,
                        int64_t C, int64_t Ho, int64_t Wo, int64_t stride, int64_t dil, int act, void* stream);
int mrfp_dwconv_dgrad(const void* dy, const float* w, void* dx, int dtype, int64_t B, int64_t H, int64_t W, int64_t Cp, int64_t C,
                      int64_t Ho, int64_t Wo, int64_t stride, int64_t dil, void* stream);
int mrfp_dwconv_wgrad(const void* x, const void* dy, float* dw, void* ws, int dtype, int64_t B, int64_t H, int64_t W, int64_t Cp,
                      int64_t C, int64_t Ho, int64_t Wo, int64_t stride, int64_t dil, void* stream);

/* BatchNorm apply + ReLU6 (reference Mobilenet.py ConvBNReLU: nn.ReLU6): y = clamp(x*A[c] + S[c], 0, 6) over the dense [npix][C]
 * tensor, and the pass mask of the fp32 PRE-activation -- bit e & 7 of byte e >> 3 = (0 < x*A + S < 6), torch's hardtanh gate --
 * in the format of mrfp_affine_fwd_relu_mask, so mrfp_stats_bwd_mask / mrfp_affine_bwd_mask consume it unchanged (16-bit, C % 8 == 0).
 * Every activation dtype, any C. */
int mrfp_affine_fwd_relu6_mask(const void* x, void* y, void* mask, int dtype, int64_t npix, int64_t C, const float* A, const float* S,
                               void* stream);
/* out = dy * mask bit, over n elements (the gate where the masked statistics / apply kernels do not apply: fp32). */
int mrfp_mask_gate(const void* dy, const void* mask, void* out, int dtype, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Test-time augmentation of the eval path (build-defined: the reference scores one forward per image, main.py:887-913).
 *
 * mrfp_prob_accum: ONE launch per (scale, flip, window) variant.  Replaces the stock chain
 *   acc[:, y0:y0+hd, x0:x0+wd] += weight * softmax(F.interpolate(flip(logits), (hd, wd), 'bilinear', align_corners=True), 1);
 *   cnt[:, y0:y0+hd, x0:x0+wd] += weight
 * (five or six passes over a [B,NC,hd,wd] fp32 tensor).  logits[B,hs,ws,ld]: low-resolution class scores in `dtype`, ld >= NC
 * channels per pixel (any pitch; 16-byte multiples are read with 16-byte loads), NC <= 32.  acc[B,H,W,NC], cnt[B,H,W]: fp32,
 * dense, read-modify-written inside the rectangle and untouched outside.  Destination pixel (y, x) of the rectangle takes the
 * align_corners=True sample of the hs x ws map at the position it has in an hd x wd resize (the arithmetic of mrfp_bilinear_fwd;
 * hs == hd and ws == wd: the identity); flip != 0 mirrors the source column (ws - 1 - column), i.e. samples flip(logits).
 * Softmax in fp32, max-subtracted.  Every destination pixel is owned by one lane, no atomics: launches on one stream give a
 * bitwise reproducible accumulator.
 *
 * mrfp_acc_argmax_hist: the closing pass.  Replaces np.argmax(acc, -1) + metrics.fast_hist (reference metrics.py:122-126) on the
 * host.  acc[npix][NC] fp32; hist / target / pred exactly as mrfp_argmax_hist (first maximum wins; labels outside 0..NC-1 are
 * ignored; hist is added to; pred uint8 [npix], optional).  Dividing by cnt does not change the arg-max and is not done.  A pixel
 * that no variant covered (cnt == 0) is the caller's error: with cnt and uncovered (int64[1], added to) given, such pixels are
 * COUNTED there so that the caller can raise; they are not hidden (their arg-max is that of whatever acc holds).
 * ------------------------------------------------------------------------------------------- */
int mrfp_prob_accum(const void* logits, int dtype, int64_t B, int64_t hs, int64_t ws, int64_t ld, float* acc, float* cnt,
                    int64_t H, int64_t W, int64_t NC, int64_t y0, int64_t x0, int64_t hd, int64_t wd, int flip, float weight,
                    void* stream);
int mrfp_acc_argmax_hist(const float* acc, const float* cnt, const int64_t* target, int64_t npix, int64_t NC, int64_t* hist,
                         uint8_t* pred, int64_t* uncovered, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Prediction path (csrc/predict.hip): label maps, validation loss and colour images without the full-resolution logits.
 * Replaces the reference's outputs = model(inputs) + np.argmax on the host + fast_hist (main.py:896-909), the val_loss its
 * evaluation bookkeeping tracks beside mIoU (utils/misc.py:139-156) and decode_segmap / get_cityscapes_labels
 * (utils_main.py:28-103); in this build, the chain mrfp_bilinear_fwd -> fp32 copy -> mrfp_argmax_hist.
 *
 * mrfp_upsample_argmax: P[B,Hi,Wi,ld] low-resolution class scores in `dtype`, NHWC, ld a multiple of the 16-byte chunk and at
 * least C rounded up to one (what mrfp_upsample_ce_fwd accepts; pad channels and chunks past the class count are never read into
 * the result), C <= 64.  For output pixel (b, y, x) of the H x W map:
 *   z_c   the align_corners=True bilinear sample of class c in fp32 (the arithmetic of mrfp_bilinear_fwd), rounded to `dtype` and
 *         widened again for the 16-bit types: the value mrfp_bilinear_fwd stores.  The predictions are therefore those of the
 *         materialised chain, pixel for pixel, in every dtype.
 *   pred  uint8 [B,H,W], optional: the first maximum of z (np.argmax's rule).
 *   conf  fp32 [B,H,W], optional: 1 / sum_c exp(z_c - max z), the largest soft-max probability.
 *   hist  int64, optional, needs target: hist[t*C + pred] += 1 for t = target[b,y,x] in 0..C-1; added to, never cleared.
 *         per_image != 0: the layout is [B][C][C], one matrix per image.
 *   loss  optional (loss_acc != NULL), needs target and ws: plain cross entropy on z; labels equal to ignore_index, < 0 or >= C
 *         are ignored.  Every workgroup writes one (sum nll, count) fp32 partial into ws (2 * mrfp_upsample_argmax_nblocks(B, H, W)
 *         floats); a one-workgroup kernel adds them in double, in a fixed order, ONTO loss_acc = double[2] (sum nll, valid
 *         pixels) on the device, which the caller owns and clears.  No floating-point atomics: runs are bitwise reproducible.
 *         The validation loss of a data set is loss_acc[0] / loss_acc[1] over all of its batches (build-defined: pixel-weighted;
 *         no valid pixel gives NaN).
 * Every output is optional on its own; none at all is refused.  Grid: (workgroups per image, B), at most 2048 workgroups;
 * mrfp_upsample_argmax_nblocks returns their number.  All argument checks happen before any launch.
 *
 * mrfp_colorize_u8: pred uint8 [npix], palette uint8 [256][3] on the device, image uint8 [npix][3] or NULL, out uint8 [npix][3].
 * image == NULL: out = palette[pred].  Otherwise out = (a * palette[pred] + (256 - a) * image + 128) >> 8 per byte in integer
 * arithmetic, 0 <= a <= 256 (256: the palette colour, 0: the image).  No pointer needs an alignment (4-byte aligned ones move
 * four pixels per lane); out must not overlap an input.
 * ------------------------------------------------------------------------------------------- */
int64_t mrfp_upsample_argmax_nblocks(int64_t B, int64_t H, int64_t W);
int mrfp_upsample_argmax(const void* P, int64_t ld, const int64_t* target, int dtype, int64_t B, int64_t Hi, int64_t Wi, int64_t H,
                         int64_t W, int64_t C, int64_t ignore_index, uint8_t* pred, float* conf, int64_t* hist, int per_image,
                         float* ws, double* loss_acc, void* stream);
int mrfp_colorize_u8(const void* pred, const void* palette, const void* image, void* out, int64_t npix, int a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MRFP_HIP_H */
