/* pixelsynth_consistency.h -- the C ABI of libpixelsynth_consistency.so, the homography consistency score (csrc/consistency.hip): the
 * reference's calc_errors_consistency_homography.py on the device.  A library of its own next to libpixelsynth_hip.so and
 * libpixelsynth_percsim.so.  Same conventions as include/pixelsynth_hip.h (int status, 0 = success; ps_consistency_last_error() says
 * why not; the last parameter is the stream). */
#ifndef PIXELSYNTH_CONSISTENCY_H
#define PIXELSYNTH_CONSISTENCY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* ---- ps_consistency: per item b of B, two views and their masks; direction 0 warps view 2 into view 1's frame, direction 1 view 1
 *   into view 2's (calc_errors_consistency_homography.py:87-98), both in one launch, then a second launch for the per-direction PSNR.
 *   view1, view2 (B, 3, H, W) read through element strides (dtype PS_DTYPE_F32 = 0, values in [0, 1], or PS_DTYPE_U8 = 1, x / 255.0f:
 *   TF.to_tensor's values).  mask1, mask2 (B, 1, H, W) contiguous, mask_dtype PS_DTYPE_F32 or PS_DTYPE_U8 (g / 255.0f).
 *   inv_maps (B, 2, 9) fp64 contiguous: per item the row-major 3 x 3 map from output to source pixel of direction 0 and of direction 1,
 *   i.e. warpPerspective's inverted matrix (the host inverts the fitted homographies).
 *   Per output pixel (x, y) of direction k: the source position in fixed point with 5 fractional bits, computed in fp64 as OpenCV's
 *   WarpPerspectiveInvoker does (per 64-column block at H, W >= 16; see csrc/consistency.hip), the 4 taps of the source view's
 *   fl32(u * 255) in BGR order (0 outside the image), weighted by the fp32 32 x 32 bilinear table; then, with m the mask of view k+1,
 *   a = fl32(warped * m) / 255, b = fl32(fl32(m * u_ref) * 255) / 255 (fp32), the per-tile fp64 sums of m sum_c (a - b)^2 and of m.
 * psnr (B, 2) f32: 10 log10(1 / mse), mse = sum m d^2 / (3 max(sum m, 1)), clamped at 100 (an empty mask scores 100).
 * percsim_mode PS_CONSISTENCY_NO_PERCSIM: percsim_in unused (NULL); PS_CONSISTENCY_PERCSIM: percsim_in (4B, H, W, 4) fp32 NHWC,
 *   16-byte aligned, channel 3 zero, pair p = 2 b + k: image p is a, image 2B + p is b, each as ((t * 2 - 1) - shift_c) / scale_c with
 *   PNet's RGB constants on the BGR-ordered values (what ps_percsim_input writes; the input of a PercSim network pass of P = 2B pairs);
 *   PS_CONSISTENCY_PERCSIM_RAW: the same with t * 2 - 1 alone (PNet.forward's input in [-1, 1]).
 *   workspace: >= ps_consistency_workspace_bytes(B, H, W) bytes of device memory.  No allocation, no synchronisation, no atomics:
 *   bit-reproducible, and an item's numbers depend neither on its place in the batch nor on B.
 * ps_consistency_workspace_bytes: host-only arithmetic; 0 for a non-positive size. */
enum { PS_CONSISTENCY_NO_PERCSIM = 0, PS_CONSISTENCY_PERCSIM = 1, PS_CONSISTENCY_PERCSIM_RAW = 2 };
size_t ps_consistency_workspace_bytes(int B, int H, int W);
int ps_consistency(const void *view1, const int64_t *strides1, const void *view2, const int64_t *strides2, int dtype, const void *mask1,
                   const void *mask2, int mask_dtype, const double *inv_maps, int B, int H, int W, int percsim_mode, float *percsim_in,
                   float *psnr, void *workspace, size_t workspace_bytes, void *stream);
/* ps_consistency_last_error: the message of this library's last failed call. */
const char *ps_consistency_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_CONSISTENCY_H */
