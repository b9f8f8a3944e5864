/* pixelsynth_vq_conv_train.h -- the C ABI of libpixelsynth_vq_conv_train.so: what makes the VQ-VAE's convolutions (vqvae2/vqvae.py)
 * differentiable around the matrix products that exist already (csrc/conv_f16x3.hip forward, csrc/conv_bwd.hip and csrc/block_train.hip
 * backward): the ReLU / space-to-depth pass that builds a grad-weight GEMM's operand, the gate that ends a grad-input pass, the fold of
 * a 3 x 3 block weight's gradient back to the 4 x 4 stride-2 weight, and the backward passes of the two 3-channel ends
 * (csrc/vq_ends.hip) -- csrc/vq_conv_train.hip.  libpixelsynth_hip.so's pinned set of exports stays as it is.  Same conventions: int
 * status, 0 = success, ps_vq_conv_train_last_error() says why not; every buffer and the workspace are the caller's; the last parameter
 * is the stream; no allocation, no synchronisation, no device-to-host copy, no atomics.  Every result is bit-identical from run to run.
 * Every buffer is fp32 and aligned to 16 bytes. */
#ifndef PIXELSYNTH_VQ_CONV_TRAIN_H
#define PIXELSYNTH_VQ_CONV_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the ReLU / pack pass -----------------------------------------------------------------------------------------------------------
 * x (B, H, W, C), C a multiple of 4, B H W C < 2^33.  a = relu ? (x < 0 ? 0 : x) : x  (a NaN stays a NaN).
 *   s2d == 0: out (B, H, W, C) = a
 *   s2d != 0: out (B, H / 2, W / 2, 4 C), channel (sy * 2 + sx) * C + c = a at pixel (2 y + sy, 2 x + sx) -- H and W even: the order
 *             in which ps_conv3x3_f16x3_ex_nhwc reads an in_s2d input.
 * out must not be x. */
int ps_vq_relu_pack_f32(const float *x, int B, int H, int W, int C, int relu, int s2d, float *out, void *stream);

/* ---- the gate pass, in place on gx, n floats (a multiple of 4) ---------------------------------------------------------------------------
 *   v = gx[i];   scale2 != NULL: v = v * scale2[1]  (the 1 / s of ps_conv3x3_bwd_prepare_f32, a power of two: exact);
 *   skip != NULL: v = v + skip[i]  (one rounding);   x != NULL: v = x[i] > 0 ? v : 0  (a select: a NaN x gives 0);   gx[i] = v. */
int ps_vq_gate_f32(float *gx, const float *x, const float *skip, const float *scale2, size_t n, void *stream);

/* ---- the fold pass: pure copies ----------------------------------------------------------------------------------------------------------
 * transposed == 0: g (Co, 3, 3, 4 Ci) -- the gradient of s2d_weight(w) in the grad-weight GEMM's layout -- to out (Co, Ci, 4, 4):
 *     out[o, c, ky, kx] = g[o, BY[ky], BY[kx], (SY[ky] * 2 + SY[kx]) * Ci + c],      BY = {0, 1, 1, 2},  SY = {1, 0, 1, 0}
 * transposed != 0: g (4 Co, 3, 3, Ci) -- the gradient of convt_weight(wt) -- to out (Ci, Co, 4, 4):
 *     out[c, o, ky, kx] = g[(SY[ky] * 2 + SY[kx]) * Co + o, DY[ky], DY[kx], c],       DY = {2, 1, 1, 0}
 * the 16 live of the 36 (block, sub-position) pairs; the other 20 are not read.  Co * Ci * 16 < 2^31. */
int ps_vq_fold_f32(const float *g, int Co, int Ci, int transposed, float *out, void *stream);

/* ---- the ends' weight and bias gradient ----------------------------------------------------------------------------------------------
 *   dW[o, c, ky, kx] = sum_{b, y, x} wide[b, y, x, o] * img[b, c, 2 y - 1 + ky, 2 x - 1 + kx]            (64, 3, 4, 4)
 * img (B, 3, H, W) NCHW, H and W even; wide has 64 channels at (H / 2, W / 2); a tap outside the frame contributes nothing.
 *   blocked != 0 (the stem): wide is given as (B, H / 4, W / 4, 256), pixel (y, x) channel o at
 *       [b, y / 2, x / 2, ((y & 1) * 2 + (x & 1)) * 64 + o]  (H and W multiples of 4);   grad_bias (64)[o] = sum wide[.., o]
 *   blocked == 0 (the head): wide is (B, H / 2, W / 2, 64) and relu(wide) is summed (applied as it is read);
 *       grad_bias (3)[c] = sum_{b, Y, X} img[b, c, Y, X]
 * The P = B (H / 2) (W / 2) < 2^31 pixels, numbered frame by frame and row by row, are cut into parts of consecutive pixels:
 *   part pixels = max(PS_VQ_CONV_TRAIN_MIN_PART, GROUPS * ceil(ceil(P / GROUPS) / PS_VQ_CONV_TRAIN_MAX_PARTS)),  parts = ceil(P / part pixels)
 * a function of P alone.  Inside a part group j of the PS_VQ_CONV_TRAIN_GROUPS groups takes the part's pixels j, j + GROUPS, ... in
 * that order, one chain of fp32 fused multiply-adds per element (taps ky, kx ascending within a pixel); the groups are added in
 * ascending order, then a second kernel adds the parts in ascending order.  The bias sums take the same walk in fp64 (the head's: a
 * pixel's four image values (2 y + j, 2 x + i), j then i ascending) and are rounded once. */
#define PS_VQ_CONV_TRAIN_MAX_PARTS 256
#define PS_VQ_CONV_TRAIN_MIN_PART 256
#define PS_VQ_CONV_TRAIN_GROUPS 16

/* The number of parts and the bytes of workspace for P pixels; both 0 for P < 1 or P >= 2^31. */
int ps_vq_conv_train_parts(long long P);
size_t ps_vq_conv_train_workspace_bytes(long long P);

int ps_vq_ends_grad_weight_f32(const float *img, const float *wide, int B, int H, int W, int blocked, float *grad_weight,
                               float *grad_bias, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the head's input gradient -----------------------------------------------------------------------------------------------------------
 * gh (B, Hh, Wh, 64)[b, y, x, o] = h[b, y, x, o] > 0 ? sum_{c, ky, kx} wt[o, c, ky, kx] * g_img[b, c, 2 y - 1 + ky, 2 x - 1 + kx] : 0
 * g_img (B, 3, 2 Hh, 2 Wh) NCHW, wt (64, 3, 4, 4) -- the transposed convolution's own weight --, h (B, Hh, Wh, 64); Wh a multiple of 16.
 * Conv2d(3, 64, 4, stride 2, padding 1) as ps_vq_stem_s2d_f32 computes it (v_mfma_f32_16x16x4_f32: exact fp32 products, one fp32 chain
 * over k = c * 16 + ky * 4 + kx ascending from 0), taps outside the frame as zeros, without a bias; the mask is a select (a NaN h gives 0). */
int ps_vq_head_grad_input_f32(const float *g_img, const float *wt, const float *h, int B, int Hh, int Wh, float *gh, void *stream);

/* ps_vq_conv_train_last_error: the message of this library's last failed call. */
const char *ps_vq_conv_train_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_VQ_CONV_TRAIN_H */
