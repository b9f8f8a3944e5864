/* pixelsynth_unet_train.h -- the C ABI of libpixelsynth_unet_train.so: the elementwise half of the depth regressor (networks/
 * architectures.py: Unet) in training -- plain nn.BatchNorm2d on the batch's statistics with an optional leaky ReLU written beside it,
 * and relu -> bilinear x2 of the concatenation of two tensors, each with its backward pass (csrc/unet_train.hip).
 * libpixelsynth_hip.so's pinned set of exports stays as it is.  Same conventions: int status, 0 = success,
 * ps_unet_train_last_error() says why not; every buffer and the workspace are the caller's; the last parameter is the stream; no
 * allocation, no synchronisation, no device-to-host copy, no atomics.  Every result is bit-identical from run to run.
 *
 * Notation: x, y, z, dy, dz, dx (N, C) channels-last fp32 -- N = B * H * W rows of a (B, C, H, W) tensor --, C a multiple of 4;
 * weight, bias, mean, var, rstd, running_mean, running_var, dweight, dbias (C) fp32; num_batches_tracked one int64.  Every buffer is
 * aligned to 16 bytes (num_batches_tracked to 8).  Sizes: N >= 1 (the running update needs N >= 2), 4 <= C <= PS_UNET_TRAIN_MAX_C,
 * N < 2^31. */
#ifndef PIXELSYNTH_UNET_TRAIN_H
#define PIXELSYNTH_UNET_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The N rows are cut into parts of consecutive rows, each a multiple of PS_UNET_TRAIN_PART_ROWS rows long (the last may be shorter): the
 * smallest multiple that gives at most PS_UNET_TRAIN_MAX_PARTS parts,
 *   rows per part = PART_ROWS * ceil(ceil(N / PART_ROWS) / MAX_PARTS),    parts = ceil(N / rows per part).
 * A function of N alone.  Inside a part a workgroup of 256 threads takes cw = min(C / 4, 64) quads of channels, so ceil((C / 4) / cw)
 * workgroups lie across the channels, and rl = 256 / cw row lanes (rounded down; the threads left over idle).  Lane l adds the part's
 * rows l, l + rl, l + 2 rl, ... in that order in fp64; the lanes of a channel are added in ascending order, then the parts in ascending
 * order by one thread per channel, and the total is rounded once. */
#define PS_UNET_TRAIN_MAX_PARTS 256
#define PS_UNET_TRAIN_PART_ROWS 256
#define PS_UNET_TRAIN_MAX_C 65536

/* Bytes of workspace the batch norm's entry points need for these sizes (device memory; one size serves all of them), and the number
 * of parts; both 0 for sizes they refuse. */
size_t ps_unet_train_workspace_bytes(int N, int C);
int ps_unet_train_parts(int N, int C);

/* Per channel S1 = sum x and S2 = sum x^2 over the N rows in fp64, then in fp64
 *   mean = S1 / N,   var = max(S2 / N - mean^2, 0)   (the biased variance; NaN stays NaN),
 * each rounded once to fp32, and rstd = 1 / sqrt(var + eps): the sum in fp32, its reciprocal root rounded once to fp32.
 * With running_mean (then running_var and num_batches_tracked are required too, and N >= 2) the module's buffers are updated in place,
 * every product and sum rounded on its own in fp32, on the fp32 mean and var:
 *   running_mean = running_mean * keep + mean * momentum          running_var = running_var * keep + (var * unbias) * momentum
 *   num_batches_tracked += 1
 * keep = (float)(1 - momentum) and unbias = (float)(N / (N - 1)) are computed in fp64 on the host and rounded once. */
int ps_bn_stats_f32(const float *x, int N, int C, float eps, float momentum, float *running_mean, float *running_var,
                    long long *num_batches_tracked, float *mean, float *var, float *rstd, void *workspace, size_t workspace_bytes,
                    void *stream);

/* scale = rstd[c] * weight[c];  shift = mean[c] * scale - bias[c];  y = x * scale - shift;  z = y > 0 ? y : slope * y
 * fp32, every operation rounded on its own; a NaN stays a NaN in both.  z may be NULL (then it is not written). */
int ps_bn_act_apply_f32(const float *x, const float *mean, const float *rstd, const float *weight, const float *bias, int N, int C,
                        float slope, float *y, float *z, void *stream);

/* The backward pass of apply(stats(x)) in x, weight and bias.  y is recomputed from x as apply computes it (the same bits):
 *   g = dy + dz * (y > 0 ? 1 : slope)   (dy or dz may be NULL: that term is absent; not both);   xhat = (x - mean) * rstd   (fp32)
 *   dbias[c] = sum over the rows of g,   dweight[c] = sum of g * xhat    (fp64 sums as above, rounded once to fp32)
 *   k1[c] = weight[c] * sum g / N,  k2[c] = weight[c] * sum g xhat / N   (fp64 on the fp64 sums, rounded once to fp32)
 *   dx = rstd * (weight * g - k1 - xhat * k2)                            (fp32)
 * g is formed inside both passes and never stored.  dx may be NULL: its pass is then not launched. */
int ps_bn_act_backward_f32(const float *x, const float *dy, const float *dz, const float *mean, const float *rstd, const float *weight,
                           const float *bias, int N, int C, float slope, float *dx, float *dweight, float *dbias, void *workspace,
                           size_t workspace_bytes, void *stream);

/* out (B, 2 H, 2 W, Ca + Cb) = bilinear x2 (align_corners = False) of relu(cat(a (B, H, W, Ca), b (B, H, W, Cb))) along the channels;
 * b may be NULL with Cb = 0.  Ca and Cb multiples of 4.  The source coordinate of output index d is max((d + 0.5) / 2 - 0.5, 0), its
 * samples i0 = floor, i1 = min(i0 + 1, n - 1), the weight of i1 the fraction w (the rule of ps_upsample_add_nhwc_f32); per output
 *   v = r00 (1 - wy)(1 - wx) + r01 (1 - wy) wx + r10 wy (1 - wx) + r11 wy wx,   r = relu(sample),  summed in that order in fp32.
 * The weights are exact in fp32.  relu keeps a NaN.  A 1 x 1 map gives relu of the pixel four times, exactly. */
int ps_relu_up2_cat_f32(const float *a, const float *b, int B, int H, int W, int Ca, int Cb, float *out, void *stream);

/* The adjoint, one call per operand: grad_in (B, H, W, Cs) from g (B, 2 H, 2 W, C) read at channels c0 .. c0 + Cs - 1, masked by the
 * operand src (B, H, W, Cs).  Input index i of n hears from the outputs 2 i - 1 .. 2 i + 2 that exist with the weights
 *   0.25 (i >= 1),   0.75 or 1 at i = 0,   0.75 or 1 at i = n - 1,   0.25 (i <= n - 2)
 * -- the forward's own, the two terms of a clamped neighbour added --; the (at most 4 x 4) products weight_row * weight_col * g are
 * added rows then columns ascending in fp32;  grad_in = src > 0 ? sum : 0  (a NaN src gives NaN). */
int ps_relu_up2_cat_backward_f32(const float *g, const float *src, int B, int H, int W, int C, int c0, int Cs, float *grad_in,
                                 void *stream);

/* ps_unet_train_last_error: the message of this library's last failed call. */
const char *ps_unet_train_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_UNET_TRAIN_H */
