/* pixelsynth_block_train.h -- the C ABI of libpixelsynth_block_train.so: what a decoder block needs in training mode between its 3 x 3
 * convolutions (pixelsynth_conv_bwd.h) and its norms (pixelsynth_norm_train.h) -- the weight and bias gradient of the 1 x 1 projection
 * on the other branch, and the adjoints of the two resampling passes that join the branches (csrc/block_train.hip).
 * libpixelsynth_hip.so's pinned set of exports stays as it is.  Same conventions: int status, 0 = success,
 * ps_block_train_last_error() says why not; every buffer and the workspace are the caller's; the last parameter is the stream; no
 * allocation, no synchronisation, no device-to-host copy, no atomics.  Every result is bit-identical from run to run.
 *
 * Every tensor is channels-last fp32 -- a pixel's channels are consecutive -- and every buffer is aligned to 16 bytes. */
#ifndef PIXELSYNTH_BLOCK_TRAIN_H
#define PIXELSYNTH_BLOCK_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the 1 x 1 convolution's weight and bias gradient ------------------------------------------------------------------------------
 * x (npix, Ci), g (npix, Co):   grad_weight[o][c] = sum_p g[p][o] * x[p][c]   (Co, Ci),     grad_bias[o] = sum_p g[p][o]   (Co)
 * Sizes: Ci and Co multiples of 16, at most PS_BLOCK_TRAIN_MAX_CHANNELS each; npix a positive multiple of 16.
 *
 * The pixels are cut into parts of consecutive pixels, every part but the last `part pixels` long:
 *   tiles       = ceil(Co / 128 or 64) * ceil(Ci / 64 or 128)   (the 64-channel chunks of g and x a workgroup pairs: two of g with one
 *                 of x when Co has an even number of chunks, else one with two when Ci has, else one with one)
 *   target      = min(PS_BLOCK_TRAIN_MAX_PARTS, max(1, 512 / tiles))
 *   part pixels = max(PS_BLOCK_TRAIN_MIN_PART, 16 * ceil((npix / 16) / target)),      parts = ceil(npix / part pixels)
 * a function of (npix, Ci, Co) alone, never of the device.  A count that is no multiple of 64 leaves its last chunk short (Co mod 64
 * or Ci mod 64 channels of it exist): the lanes past the count multiply zeros and store nothing.  Inside a part the PS_BLOCK_TRAIN_WAVES wavefronts of a workgroup take
 * the groups of four consecutive pixels in turn (wavefront w the groups w, w + WAVES, ...); a wavefront accumulates its groups in
 * ascending order on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32: fp32 fused multiply-adds, no reduced-precision product), the
 * wavefronts are added in ascending order, and a second kernel adds the parts in ascending order (with one part the first kernel
 * writes the result itself).  The bias sums come from the same read of g: per wavefront the pixels p = 0, 1, 2, 3 mod 4 of its groups
 * in four chains, then those four, the wavefronts and the parts in ascending order. */
#define PS_BLOCK_TRAIN_MAX_PARTS 256
#define PS_BLOCK_TRAIN_MIN_PART 512
#define PS_BLOCK_TRAIN_WAVES 8
#define PS_BLOCK_TRAIN_MAX_CHANNELS 256

/* The number of parts, and the bytes of workspace (device memory) ps_conv1x1_grad_weight_f32 needs; both 0 for sizes it refuses. */
int ps_conv1x1_grad_weight_parts(size_t npix, int Ci, int Co);
size_t ps_conv1x1_grad_weight_workspace_bytes(size_t npix, int Ci, int Co);

/* grad_bias may be NULL (then it is not computed). */
int ps_conv1x1_grad_weight_f32(const float *x, const float *g, size_t npix, int Ci, int Co, float *grad_weight, float *grad_bias,
                               void *workspace, size_t workspace_bytes, void *stream);

/* ---- the adjoints of the resampling passes ------------------------------------------------------------------------------------------
 * Both are gathers: a thread owns four channels of one pixel of grad_in and sums what the forward pass sent out from that pixel, in
 * a fixed order -- rows of g ascending, columns ascending inside a row -- each term one rounded product w * g added to a sum that
 * starts at 0.resample(a) + resample(b) is linear and symmetric in a and b, so one adjoint serves both.
 *
 * ps_upsample_add_bwd_nhwc_f32: g (B, 2H, 2W, C) -> grad_in (B, H, W, C), the adjoint of ps_upsample_add_nhwc_f32's bilinear x2
 * (align_corners = False).  Per axis input index i (of n) hears from output index
 *   2i - 1 (i >= 1) with 0.25,     2i with 0.75 (1 for i = 0: the clamp),     2i + 1 with 0.75 (1 for i = n - 1: there the forward's
 *   two samples i0 = i1 = i coincide and their weights 0.75 + 0.25 fold onto it),     2i + 2 (i <= n - 2) with 0.25
 * and w is the product of the row's and the column's weight (exact in fp32): at most 4 x 4 terms.  The forward's weight-0 sample of
 * output 0 (input 1 at the clamp) is no term.  C a multiple of 4; B, H, W >= 1.
 *
 * ps_pool_add_bwd_nhwc_f32: g (B, H/2, W/2, C) -> grad_in (B, H, W, C), the adjoint of avg_pool2d(., 3, 2, 1) with the padding counted in
 * the divisor, as ps_pool_add_nhwc_f32 computes it.  Input pixel (yy, xx) sums g[yo][xo] over the in-range outputs with
 * |2 yo - yy| <= 1 and |2 xo - xx| <= 1 -- 1, 2 or 4 of them -- in ascending (yo, xo) and multiplies the sum once by the forward's
 * 1.0f / 9.0f.  H and W even and >= 2, C a multiple of 4. */
int ps_upsample_add_bwd_nhwc_f32(const float *g, int B, int H, int W, int C, float *grad_in, void *stream);
int ps_pool_add_bwd_nhwc_f32(const float *g, int B, int H, int W, int C, float *grad_in, void *stream);

/* ps_block_train_last_error: the message of this library's last failed call. */
const char *ps_block_train_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_BLOCK_TRAIN_H */
