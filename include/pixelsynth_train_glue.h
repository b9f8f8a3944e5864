/* pixelsynth_train_glue.h -- the C ABI of libpixelsynth_train_glue.so: the full-resolution passes that sit between the units of the
 * generator's training step (csrc/train_glue.hip; the reference's models/z_buffermodel.py forward_image :303-311 and get_combined
 * :703-708) -- the depth head behind the regressor, and the blend of the reprojected features with the decoded codes joined with the
 * mask channel and written as the decoder's channels-last input -- each forward and backward.
 * libpixelsynth_hip.so's pinned set of exports stays as it is.  Same conventions: int status, 0 = success,
 * ps_train_glue_last_error() says why not; every buffer is the caller's; the last parameter is the stream; no allocation, no
 * synchronisation, no device-to-host copy, no atomics.
 *
 * Every pass is elementwise: a lane owns one pixel (sample, row, column) and a pixel's results depend on nothing but its own operands --
 * not on B, not on its place in the batch, not on the launch.  Every operation is rounded on its own (-ffp-contract=off). */
#ifndef PIXELSYNTH_TRAIN_GLUE_H
#define PIXELSYNTH_TRAIN_GLUE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_GLUE_DEPTH_RANGE 0   /* depth = s * (max_z - min_z) + min_z */
#define PS_GLUE_DEPTH_INVERSE 1 /* depth = 1 / (s * 10 + 0.01f)        */

/* gen_fs, input_gt (B,3,H,W) dense NCHW fp32; background_mask (B,H,W) bytes, nonzero = background; out (B,H,W,4) fp32, aligned to 16
 * bytes.  With bg = mask ? 1.0f : 0.0f and fg = 1.0f - bg (so both are 0.0f or 1.0f):
 *   out[b,y,x,c] = gen_fs[b,c,y,x] * fg + input_gt[b,c,y,x] * bg      c < 3   (two products, one addition: a NaN or an infinity in
 *                                                                             the operand the mask switches off still gives NaN)
 *   out[b,y,x,3] = fg
 * Sizes: B, H, W >= 1, B H W < 2^31. */
int ps_combine_mask_nhwc_f32(const float *gen_fs, const float *input_gt, const uint8_t *background_mask, int B, int H, int W, float *out,
                             void *stream);

/* Its backward pass: grad_out (B,H,W,4) fp32 aligned to 16 bytes -> grad_gen (B,3,H,W) dense NCHW,
 *   grad_gen[b,c,y,x] = grad_out[b,y,x,c] * fg        (a product: a NaN stays one where the mask is set)
 * input_gt and the mask get no gradient; channel 3 of grad_out is not read for a value. */
int ps_combine_mask_nhwc_backward_f32(const float *grad_out, const uint8_t *background_mask, int B, int H, int W, float *grad_gen,
                                      void *stream);

/* The depth head: raw, depth, pred_img of N fp32 values each.
 *   s = 1 / (1 + expf(-raw))                          (a true division)
 *   depth = s * float(max_z - min_z) + float(min_z)   (PS_GLUE_DEPTH_RANGE; the difference is taken in double on the host)
 *   depth = 1 / (s * 10 + 0.01f)                      (PS_GLUE_DEPTH_INVERSE; min_z and max_z are not read)
 *   pred_img = depth / 5 - 1                          (a true division)
 * 1 <= N < 2^31; min_z, max_z finite in PS_GLUE_DEPTH_RANGE. */
int ps_depth_head_forward_f32(const float *raw, int mode, double min_z, double max_z, long long N, float *depth, float *pred_img,
                              void *stream);

/* Its backward pass: s (and, in PS_GLUE_DEPTH_INVERSE, depth) recomputed from raw as the forward computes them; with t = s * (1 - s)
 *   grad_raw = (grad_depth * float(max_z - min_z)) * t                   (PS_GLUE_DEPTH_RANGE)
 *   grad_raw = -(((grad_depth * 10) * t) * (depth * depth))              (PS_GLUE_DEPTH_INVERSE) */
int ps_depth_head_backward_f32(const float *raw, const float *grad_depth, int mode, double min_z, double max_z, long long N,
                               float *grad_raw, void *stream);

/* ps_train_glue_last_error: the message of this library's last failed call. */
const char *ps_train_glue_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_TRAIN_GLUE_H */
