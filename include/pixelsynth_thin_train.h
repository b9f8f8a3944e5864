/* pixelsynth_thin_train.h -- the C ABI of libpixelsynth_thin_train.so: the backward passes of the refinement decoder's THIN convolutions,
 * the layers that join a wide side of Cw channels with a thin side of T channels (block 0: 4 -> 64, 3 x 3 and 1 x 1; block 7: 128 -> 3,
 * 3 x 3 and 1 x 1), csrc/thin_train.hip.  Their forward passes are the no-grad kernels of libpixelsynth_hip.so (csrc/conv_thin.hip,
 * csrc/conv1x1.hip), whose pinned set of exports stays as it is; the gradient to the thin input of a 4 -> Cw layer is those kernels on
 * the flipped, transposed weight.  What is new here: the gradient to the wide input of a Cw -> T layer (ps_thin_expand_f32), the weight
 * and bias gradient of all four layers (ps_thin_grad_weight_f32), and the bias add that completes a forward pass (ps_thin_add_bias_f32).
 * Same conventions as pixelsynth_norm_train.h and pixelsynth_block_train.h: int status, 0 = success, ps_thin_train_last_error() says
 * why not; every buffer and the workspace are the caller's; the last parameter is the stream; no allocation, no synchronisation, no
 * device-to-host copy, no atomics.  Every result is bit-identical from run to run.
 *
 * Every tensor is channels-last fp32 -- a pixel's channels are consecutive: (B, H, W, C).  The wide tensors (Cw channels, a multiple of
 * 32, at most PS_THIN_TRAIN_MAX_WIDE) and the weights are aligned to 16 bytes; a thin tensor (T channels, 1 .. 4) is aligned to 16 bytes
 * where T = 4 and to 4 bytes otherwise: the 12-byte pixels of a T = 3 map are read one float at a time.  k is 1 or 3, the padding k / 2,
 * the stride 1; tap t = ky k + kx has the offset off(t) = (ky - k / 2, kx - k / 2).  B H W < 2^31. */
#ifndef PIXELSYNTH_THIN_TRAIN_H
#define PIXELSYNTH_THIN_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_THIN_TRAIN_MAX_WIDE 256
#define PS_THIN_TRAIN_MAX_PARTS 256
#define PS_THIN_TRAIN_MIN_PART 1024
#define PS_THIN_TRAIN_GROUPS 32

/* ---- wide from thin: the gradient to the input of a Cw -> T layer ---------------------------------------------------------------------
 * g (B, H, W, T), w [k k][T][Cw]:   out[p][c] = sum_t sum_j w[t][j][c] * g[p + off(t)][j]     (B, H, W, Cw)
 * One pass over the wide output: a thread owns four channels of four neighbouring pixels of a row and stores them once.  The sum of an
 * element starts at 0 and takes one fused multiply-add per term, the taps t ascending and inside a tap the thin channels j ascending;
 * a tap outside the frame is no term (it is skipped, not multiplied by zero).  Frames do not mix: a frame's result is the same bits
 * wherever it stands in the batch.  For grad_input of y = conv(x, W), W (T, Cw, k, k):  w[t][j][c] = W[j][c][k k - 1 - t].
 * W a multiple of 4. */
int ps_thin_expand_f32(const float *g, const float *w, int B, int H, int W, int T, int Cw, int k, float *out, void *stream);

/* ---- the weight and bias gradient of all four layers ---------------------------------------------------------------------------------
 * thin (B, H, W, T), wide (B, H, W, Cw):   grad_weight[t][j][c] = sum_p thin[p + s off(t)][j] * wide[p][c]     [k k][T][Cw]
 * over the pixels p of every frame whose neighbour p + s off(t) lies inside the frame; taps outside contribute nothing.
 *   wide_is_g = 1 (a T -> Cw layer: thin is its input x, wide the gradient of its output):  s = +1,  grad_bias[c] = sum_p wide[p][c]  (Cw)
 *   wide_is_g = 0 (a Cw -> T layer: wide is its input x, thin the gradient of its output):  s = -1,  grad_bias[j] = sum_p thin[p][j]  (T)
 * so that grad_weight[t][j][c] is dL/dW[c][j][ky][kx] of the first and dL/dW[j][c][ky][kx] of the second.  The wide tensor is read
 * exactly once (each workgroup reads 32 of its channels); grad_bias comes from the same pass and may be NULL.
 *
 * The order of summation.  The pixels 0 .. B H W - 1 (frames, rows, columns) are cut into parts of consecutive pixels:
 *   part pixels = max(PS_THIN_TRAIN_MIN_PART, 32 * ceil(ceil(B H W / 32) / PS_THIN_TRAIN_MAX_PARTS)),   parts = ceil(B H W / part pixels)
 * -- at most PS_THIN_TRAIN_MAX_PARTS, a function of B H W alone, never of the device; the last part may be shorter.  Inside a part
 * [lo, hi) group q of PS_THIN_TRAIN_GROUPS takes the pixels lo + q, lo + q + 32, ... in ascending order: per element one chain of fp32
 * fused multiply-adds that starts at 0.  The 32 groups are added in ascending order, the first kernel writes one slab per part to the
 * workspace, and a second kernel adds the parts in ascending order (with one part: it copies).  A term of grad_weight passes through at
 * most ceil(part pixels / 32) + 32 + parts roundings.  grad_bias takes the same walk in fp64 -- pixels, groups, parts -- and is rounded
 * to fp32 once at the end: the sums of a gradient cancel, and fp32 partial sums would cost them digits that four adds per pixel save. */
int ps_thin_train_parts(int B, int H, int W, int Cw, int T, int k);                /* 0 for sizes ps_thin_grad_weight_f32 refuses */
size_t ps_thin_train_workspace_bytes(int B, int H, int W, int Cw, int T, int k);   /* likewise */
int ps_thin_grad_weight_f32(const float *thin, const float *wide, int B, int H, int W, int Cw, int T, int k, int wide_is_g,
                            float *grad_weight, float *grad_bias, void *workspace, size_t workspace_bytes, void *stream);

/* ---- y[p][c] += bias[c], one rounded add per element, in place: y (npix, C), any C >= 1 (16 bytes per lane where C is a multiple of 4) */
int ps_thin_add_bias_f32(float *y, const float *bias, size_t npix, int C, void *stream);

/* ps_thin_train_last_error: the message of this library's last failed call. */
const char *ps_thin_train_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_THIN_TRAIN_H */
