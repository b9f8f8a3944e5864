/* pixelsynth_norm_train.h -- the C ABI of libpixelsynth_norm_train.so: the noise-conditioned batch norm of the refinement decoder in
 * training mode (csrc/norm_train.hip; the reference's bn.forward with manual_bn / fused_bn, models/layers/normalization.py:114-200) --
 * the batch statistics with the update of the stored ones, the normalisation (+ ReLU) on them, and the backward pass through both.
 * libpixelsynth_hip.so's pinned set of exports stays as it is.  Same conventions: int status, 0 = success,
 * ps_norm_train_last_error() says why not; every buffer and the workspace are the caller's; the last parameter is the stream; no
 * allocation, no synchronisation, no device-to-host copy, no atomics.  Every result is bit-identical from run to run.
 *
 * Notation: x, y, dy, dx (B, HW, C) channels-last fp32, C a multiple of 4; gain, bias, dgain, dbias (B, C) contiguous; mean, var, rstd,
 * pend, stored_mean, stored_var (C); N = B * HW.  Every buffer is aligned to 16 bytes.  Sizes: B, HW, C >= 1, C % 4 == 0,
 * C <= PS_NORM_TRAIN_MAX_C, HW * C < 2^31 (32-bit element counts per frame), B * HW < 2^31. */
#ifndef PIXELSYNTH_NORM_TRAIN_H
#define PIXELSYNTH_NORM_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The HW rows of every frame are cut into parts of consecutive rows, each a multiple of PS_NORM_TRAIN_PART_ROWS rows long (the last
 * one of a frame may be shorter): the smallest multiple that gives a frame at most max(1, PS_NORM_TRAIN_MAX_PARTS / B) parts,
 *   rows per part = PART_ROWS * ceil(ceil(HW / PART_ROWS) / max(1, MAX_PARTS / B)),    parts per frame = ceil(HW / rows per part).
 * A function of B and HW alone; no part spans two frames.  A sum is accumulated in fp64 in a fixed order inside a part and the parts
 * are added in ascending order.
 *
 * Inside a part (tests/_norm_train_ref.py restates this): a workgroup of 256 threads takes cw = min(C / 4, 64) quads of channels, so
 * ceil((C / 4) / cw) workgroups lie across the channels (the last may take fewer quads), and rl = 256 / cw row lanes (rounded down; the
 * 256 - cw rl threads left over idle).  Lane l takes the part's rows l, l + rl, l + 2 rl, ...: blocks of four of them through two
 * register sets in turn, a block's loads issued before the block in front of it is used, for as long as a whole block lies inside the
 * part; the rows left, at most three, one at a time.  The parts of a sum are added 64 at a time (a batch is staged while the one before
 * it is added), from the first part of the sum on -- of all parts for the statistics, of each frame's parts for dgain and dbias -- by
 * workgroups of 32 channels, ceil(C / 32) of them (the last may have fewer channels). */
#define PS_NORM_TRAIN_MAX_PARTS 512
#define PS_NORM_TRAIN_PART_ROWS 512
#define PS_NORM_TRAIN_MAX_C 65536

/* Bytes of workspace the entry points below need for these sizes (device memory; one size serves all of them), and the number of
 * parts, B * parts per frame; both 0 for sizes they refuse. */
size_t ps_norm_train_workspace_bytes(int B, int HW, int C);
int ps_norm_train_parts(int B, int HW, int C);

/* Per channel S1 = sum x and S2 = sum x^2 over the N rows in fp64 (the square of an fp32 value is exact there), then in fp64
 *   mean = S1 / N,   var = max(S2 / N - mean^2, 0)   (the biased variance the reference uses and stores, clamped at 0; NaN stays NaN),
 * each rounded once to fp32, and rstd = 1 / sqrt(var + eps): the sum in fp32, its reciprocal root rounded once to fp32.
 * The stored statistics are updated in place, every product and sum rounded on its own in fp32:
 *   stored_mean = stored_mean * keep + (mean + pend) * momentum          stored_var = stored_var * keep + var * momentum
 * (keep, momentum) = (1 - momentum, momentum) is the running average, (1, 1) the standing sum.  pend (C) may be NULL (then nothing
 * is added): a convolution bias still missing from x.  It goes into the stored mean only; `mean` is that of x as passed. */
int ps_norm_train_stats_f32(const float *x, const float *pend, int B, int HW, int C, float eps, float keep, float momentum,
                            float *stored_mean, float *stored_var, float *mean, float *var, float *rstd, void *workspace,
                            size_t workspace_bytes, void *stream);

/* scale = rstd[c] * gain[b][c];  shift = mean[c] * scale - bias[b][c];  v = x * scale - shift;  y = relu ? (v < 0 ? 0 : v) : v
 * fp32, every operation rounded on its own (the reference's fused_bn in its order); a NaN stays a NaN through the ReLU. */
int ps_norm_train_apply_f32(const float *x, const float *mean, const float *rstd, const float *gain, const float *bias, int B, int HW,
                            int C, int relu, float *y, void *stream);

/* The backward pass of apply(stats(x)) in x, gain and bias.  v is recomputed from x as apply computes it (the same bits), so y is
 * not needed:   g = relu ? (v > 0 ? dy : 0) : dy   (a NaN v with relu gives g = NaN, not 0);   xhat = (x - mean) * rstd   (fp32)
 *   dbias[b][c] = sum over the frame's rows of g,   dgain[b][c] = sum of g * xhat    (fp64 sums, rounded once to fp32)
 *   k1[c] = sum_b gain[b][c] * dbias[b][c] / N,  k2[c] = sum_b gain[b][c] * dgain[b][c] / N   (fp64 on the fp64 sums, ascending b,
 *                                                                                                rounded once to fp32)
 *   dx = rstd * (gain * g - k1 - xhat * k2)                                                     (fp32)
 * dx may be NULL (the input needs no gradient): its pass is then not launched, dgain and dbias are the same bits. */
int ps_norm_train_backward_f32(const float *x, const float *dy, const float *mean, const float *rstd, const float *gain,
                               const float *bias, int B, int HW, int C, int relu, float *dx, float *dgain, float *dbias,
                               void *workspace, size_t workspace_bytes, void *stream);

/* ps_norm_train_last_error: the message of this library's last failed call. */
const char *ps_norm_train_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_NORM_TRAIN_H */
