/* pixelsynth_lmconv_bwd.h -- the C ABI of libpixelsynth_lmconv_bwd.so: the backward pass of the locally masked convolution
 * (csrc/lmconv_bwd.hip; the reference's _locally_masked_conv2d.backward, models/lmconv/locally_masked_convolution.py:52-93) -- the
 * gradients with respect to weight and bias, and the adjoint mask that turns the gradient with respect to the input into a locally
 * masked convolution of its own, run on ps_lmconv_forward_f32.  A library of its own beside libpixelsynth_hip.so, whose pinned set
 * of exports it leaves as it is.  Same conventions: int status, 0 = success, ps_lmconv_bwd_last_error() says why not; every buffer
 * and the workspace are the caller's; the last parameter is the stream; no allocation, no synchronisation, no device-to-host copy,
 * no atomics.  Every result is bit-identical from run to run.
 *
 * Notation: x (B,Ci,H,W), g = grad_y (B,Co,H,W), mask m[b,t,l] (B|1,9,L) with L = H*W and a batch stride of 9*L or 0 (one mask for the
 * whole batch), weight (Co,Ci,3,3); off(t) = ((t/3 - 1)*dilation, (t%3 - 1)*dilation); padding = dilation; xpad is x with zeros around
 * the grid. */
#ifndef PIXELSYNTH_LMCONV_BWD_H
#define PIXELSYNTH_LMCONV_BWD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The reduction over the B*L locations is split into at most this many parts, each one fused-multiply-add chain per element, whose
 * partial results are added in ascending order of the part: the most additions a result passes besides its chain. */
#define PS_LMCONV_BWD_MAX_PARTS 64

/* Bytes of workspace ps_lmconv_grad_weight_f32 needs for these sizes (device memory, 256-byte aligned); 0 for sizes it refuses. */
size_t ps_lmconv_bwd_workspace_bytes(int B, int Ci, int Co, int H, int W);

/* grad_weight[o,c,t] = sum_{b,l} g[b,o,l] * (m[b,t,l] * xpad[b,c,l+off(t)])      (Co,Ci,3,3), summed over the batch
 * grad_bias[o]       = sum_{b,l} g[b,o,l]                                         (Co)
 * Either output may be NULL (not both); x and mask may be NULL where grad_weight is.  All sizes >= 1, B*H*W <= 2^30, dilation >= 1.
 * grad_weight: channels-last copies of g and x, padded with zeros to 16 channels, are made in the workspace; a GEMM over the B*L
 * locations on v_mfma_f32_16x16x4_f32 (exact fp32: a fused-multiply-add chain in ascending location), the mask value multiplied into
 * the shifted row of x first (one rounding), the locations split into parts <= PS_LMCONV_BWD_MAX_PARTS consecutive ranges whose
 * partial tiles a second kernel adds in ascending order.  A tap that lies outside the grid contributes an exact 0.
 * grad_bias: one workgroup per channel, thread t over locations t, t + 256, ... in that order, then a fixed pairwise tree. */
int ps_lmconv_grad_weight_f32(const float *x, const float *grad_y, const float *mask, size_t mask_batch_stride, int B, int Ci, int Co,
                              int H, int W, int dilation, float *grad_weight, float *grad_bias, void *workspace,
                              size_t workspace_bytes, void *stream);

/* adjoint[b,t,p] = mask[b, 8-t, p+off(t)] where p+off(t) lies in the grid, 0 elsewhere: (Bm,9,L) -> (Bm,9,L), Bm = 1 or the batch.
 * With it grad_x = lmconv(g, adjoint, W', no bias, the same dilation), W'[c,o,t] = W[o,c,8-t]  (ps_lmconv_forward_f32). */
int ps_lmconv_adjoint_mask_f32(const float *mask, int Bm, int H, int W, int dilation, float *adjoint, void *stream);

/* ps_lmconv_bwd_last_error: the message of this library's last failed call. */
const char *ps_lmconv_bwd_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_LMCONV_BWD_H */
