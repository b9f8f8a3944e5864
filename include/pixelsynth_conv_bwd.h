/* pixelsynth_conv_bwd.h -- the C ABI of libpixelsynth_conv_bwd.so: the backward pass of the split-fp16 3 x 3 / stride 1 / pad 1
 * convolution (csrc/conv_bwd.hip; the forward is csrc/conv_f16x3.hip behind ps_conv3x3_f16x3_ex_nhwc of pixelsynth_hip.h).  A library
 * of its own beside libpixelsynth_hip.so, whose pinned set of exports it leaves as it is.  Same conventions: int status, 0 = success,
 * ps_conv_bwd_last_error() says why not; every buffer and the workspace are the caller's; the last parameter is the stream; no
 * allocation, no synchronisation, no device-to-host copy, no atomics.  Every result is bit-identical from run to run, on every card.
 *
 * Notation: x (B,H,W,Ci) fp32, g = grad_y (B,H,W,Co) fp32, weight (Co,3,3,Ci); tap t = 3 ky + kx reads xpad[b, y + ky - 1, x + kx - 1],
 * xpad is x with zeros around the frame.  H and W multiples of 16, Ci and Co multiples of 64, H*W*max(Ci,Co) < 2^31, B*H*W <= 2^30.
 *
 * The operand split of the forward (v = hi + lo, hi = fp16(v), lo = fp16(v - hi)) keeps 22 bits only while lo is a normal fp16, that is
 * for |v| >= 2^-3; gradients are routinely 1e-4 .. 1e-8.  So grad_y is multiplied by a power of two s first (exact) and the results by
 * 1 / s afterwards (exact):  s = 2^(15 - e) with max|g| = f * 2^e, f in [0.5, 1), so that max|g * s| lies in [2^14, 2^15); the exponent
 * 15 - e is held inside [-126, 126] (s and 1 / s stay normal fp32 numbers); s = 1 when the maximum is 0 or not finite.  s lives on the
 * device (scale2 = {s, 1 / s}) and is never read back.
 *
 * One backward pass:
 *     ps_conv3x3_bwd_prepare_f32      g -> scale2, g_scaled = g * s, grad_bias
 *     ps_conv3x3_grad_weight_f16x3    x, g_scaled, scale2 -> grad_weight
 *     grad_x: ps_conv3x3_f16x3_ex_nhwc (pixelsynth_hip.h) on g_scaled with the flipped, transposed weight W'[c,t,o] = W[o,8-t,c],
 *             then ps_conv3x3_bwd_unscale_f32 on its output. */
#ifndef PIXELSYNTH_CONV_BWD_H
#define PIXELSYNTH_CONV_BWD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The reduction over the pixels is split into at most this many parts of consecutive pixel tiles (4 rows x 16 pixels each), each one
 * chain of fp32 sums per element, whose partial results are added in ascending order of the part.  The number of parts is a function of
 * (B, H, W, Ci, Co) alone -- never of the device:
 *   tiles          = B (H / 4) (W / 16), numbered frame by frame, row of tiles by row of tiles
 *   tiles per part = max(8, ceil(tiles / min(PS_CONV_BWD_MAX_PARTS, ceil(512 / ((Co / 64) (Ci / 64))))))
 *   parts          = ceil(tiles / tiles per part)
 * Part p takes the tiles p * tiles per part .. ; the last part may be shorter, and a part may span two frames.  Every part is worked
 * on by (Co / 64) (Ci / 64) workgroups, one per 64 x 64 block of channels. */
#define PS_CONV_BWD_MAX_PARTS 256

/* Bytes of workspace the calls below need for these sizes (device memory, 256-byte aligned; one workspace serves prepare and
 * grad_weight, which run one after the other); 0 for sizes they refuse. */
size_t ps_conv3x3_bwd_workspace_bytes(int B, int H, int W, int Ci, int Co);

/* The number of parts ps_conv3x3_grad_weight_f16x3 splits the pixels of these sizes into (1 .. PS_CONV_BWD_MAX_PARTS); 0 for sizes it
 * refuses. */
int ps_conv3x3_bwd_parts(int B, int H, int W, int Ci, int Co);

/* One pass over g for max|g| and the per-channel sums, then scale2 = {s, 1 / s} (two floats on the device), then g_scaled = g * s
 * (B,H,W,Co).  grad_bias (Co) or NULL: grad_bias[o] = sum_{b,y,x} g[b,y,x,o] of the UNSCALED g -- the pixels cut into at most 256
 * consecutive ranges of at least 64; inside a range sixteen interleaved chains in ascending pixel order, joined by a fixed tree (chain i
 * with chain i + 8, then + 4, + 2, + 1); the ranges as four interleaved chains in ascending order joined as (0 + 1) + (2 + 3).
 *   pixels per range = max(64, ceil(B H W / 256)),     ranges = ceil(B H W / pixels per range)
 * (a range whose length is no multiple of 16 gives its chains unequal lengths).  Every range leaves one maximum per 64 channels of Co.
 * g_scaled must not be g. */
int ps_conv3x3_bwd_prepare_f32(const float *g, int B, int H, int W, int Co, float *g_scaled, float *scale2, float *grad_bias,
                               void *workspace, size_t workspace_bytes, void *stream);

/* grad_weight[o,t,c] = (1 / s) * sum_{b,y,x} g_scaled[b,y,x,o] * xpad[b, y + ky - 1, x + kx - 1, c]          (Co,3,3,Ci)
 * A GEMM over the pixels on v_mfma_f32_32x32x16_f16, both operands split as the forward splits them, every product three MFMAs
 * (g.lo * x.hi, g.hi * x.lo, g.hi * x.hi) summed in fp32; a workgroup owns 64 x 64 channels x 9 taps of one part.  A tap outside the
 * frame contributes an exact 0.  *overflow is set to 1 where an |x| > 65000 or a NaN of x is met (the result is then wrong), as the
 * forward sets it; it is never cleared here. */
int ps_conv3x3_grad_weight_f16x3(const float *x, const float *g_scaled, const float *scale2, int B, int H, int W, int Ci, int Co,
                                 float *grad_weight, int *overflow, void *workspace, size_t workspace_bytes, void *stream);

/* y[i] *= 1 / s in place, i < n; n a multiple of 4, y aligned to 16 bytes. */
int ps_conv3x3_bwd_unscale_f32(float *y, size_t n, const float *scale2, void *stream);

/* ps_conv_bwd_last_error: the message of this library's last failed call. */
const char *ps_conv_bwd_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_CONV_BWD_H */
