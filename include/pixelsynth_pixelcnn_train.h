/* pixelsynth_pixelcnn_train.h -- the C ABI of libpixelsynth_pixelcnn_train.so: what runs between the masked convolutions when the
 * PixelCNN trains (csrc/pixelcnn_train.hip; the reference's models/lmconv/layers.py gated_resnet and PONO, models/lmconv/utils.py
 * concat_elu) -- positional normalisation + skip + activation, the gate of a gated block, each forward and backward, and the backward
 * pass of the cross entropy of given codes (the forward is ps_code_nll_f32 of include/pixelsynth_nll.h).
 * libpixelsynth_hip.so's pinned set of exports stays as it is.  Same conventions: int status, 0 = success,
 * ps_pixelcnn_train_last_error() says why not; every buffer is the caller's; the last parameter is the stream; no allocation, no
 * synchronisation, no device-to-host copy, no atomics.
 *
 * Tensors are fp32.  x, y, vg, u and their gradients are dense NCHW, (B,C,H,W): a LOCATION is one (sample, row, column), N = B H W of
 * them, L = H W per sample, and a location's C channels lie L values apart.  `skip` (and its gradient) is either dense NCHW
 * (PS_PCT_NCHW) or dense (B,H,W,C) (PS_PCT_NHWC: what a 1 x 1 `nin` leaves behind its movedim view).
 *
 * Every sum over a location's channels is taken in fp64 and rounded once: four chains, chain k adding the channels k, k + 4, k + 8, ...
 * in ascending order, joined as (s0 + s1) + (s2 + s3).  A launch gives a location one lane (N >= PS_PCT_WIDE_LOCATIONS: the lane walks
 * the four chains) or four (below: lane k of wavefront k walks chain k, the four meet in LDS); the sums are the same bits either way, so a
 * location's results depend on neither B, nor its place in the batch, nor the launch.  Both forms stream the channels (two walks of
 * the operand per pass); there is no register-resident form and so no limit on C but PS_PCT_MAX_CHANNELS. */
#ifndef PIXELSYNTH_PIXELCNN_TRAIN_H
#define PIXELSYNTH_PIXELCNN_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_PCT_NCHW 0
#define PS_PCT_NHWC 1
#define PS_PCT_ACT_NONE 0            /* y = z                                   (B,C,H,W)  */
#define PS_PCT_ACT_ELU 1             /* y = elu(z)                              (B,C,H,W)  */
#define PS_PCT_ACT_CELU 2            /* y = elu(z) | elu(-z) along the channels (B,2C,H,W) */
#define PS_PCT_MAX_CHANNELS 65536
#define PS_PCT_WIDE_LOCATIONS 262144 /* from this many locations on a lane owns a location (1024 workgroups: 16 wavefronts for each
                                      * of 256 compute units); below, four lanes share one */
#define PS_PCT_EPS 1e-5              /* PONO's, inside the root */
#define PS_PCT_GROUP_OBSERVED 1      /* bits of `groups` below */
#define PS_PCT_GROUP_SAMPLED 2

/* Lanes a launch over N locations gives to each location: 4 below PS_PCT_WIDE_LOCATIONS, else 1; 0 for N < 1. */
int ps_pixelcnn_train_lanes(long long N);

/* z = (norm ? PONO(x) : x) [+ skip],  y = act(z).
 * PONO, per location: with K = the location's channel 0, S1 = sum (x - K), S2 = sum (x - K)^2 in fp64 (the differences of fp32 values
 * within 2^29 of each other are exact there; K is one of the samples, so the subtraction below cancels C-fold at the worst),
 *   mean = K + S1 / C,   var = max((S2 - S1^2 / C) / (C - 1), 0)  (unbiased; NaN stays NaN),   rstd = 1 / sqrt(var + PS_PCT_EPS)
 * in fp64, mean and rstd each rounded once to fp32 -- outputs (N values each) when norm is set, the backward pass takes them.
 * Then in fp32, every operation rounded on its own: xh = (x - mean) * rstd, z = xh + skip, elu(z) = z > 0 ? z : expm1f(z).
 * skip may be NULL.  Sizes: B, L >= 1, B L < 2^31, 2 <= C <= PS_PCT_MAX_CHANNELS where norm is set, 1 <= C otherwise. */
int ps_norm_act_forward_f32(const float *x, const float *skip, int skip_layout, int B, int C, int L, int norm, int act, float *y,
                            float *mean, float *rstd, void *stream);

/* Its backward pass.  z is recomputed from x, skip, mean and rstd as the forward computes it (the same bits); dy is (B,C,H,W), or
 * (B,2C,H,W) for PS_PCT_ACT_CELU (g1 = its first C channels, g2 = the others).  With elu'(t) = t > 0 ? 1 : expf(t):
 *   dz = dy                                     (no activation)
 *   dz = dy * elu'(z)                           (elu)
 *   dz = g1 * elu'(z) - g2 * elu'(-z)           (concatenated)                                      (fp32)
 *   dskip = dz                                  (written in skip's layout; NULL: not wanted)
 *   dx = dz                                     (norm off)
 *   m1 = sum dz / C,  m2 = sum dz * xh / (C - 1)             (products and sums in fp64, each quotient rounded once to fp32)
 *   dx = rstd * ((dz - m1) - xh * m2)                                                                (fp32)
 * dx may be NULL (not wanted); dx and dskip may not both be NULL. */
int ps_norm_act_backward_f32(const float *x, const float *skip, int skip_layout, const float *dy, const float *mean, const float *rstd,
                             int B, int C, int L, int norm, int act, float *dx, float *dskip, void *stream);

/* The gate of a gated block: vg (B,2C,H,W) as conv_out leaves it, v = its first C channels, g = the others; u (B,C,H,W).
 *   out = u + PONO(v) * sigmoid(g),   sigmoid(g) = 1 / (1 + expf(-g))  (a true division)
 * PONO as above; mean and rstd (N values each) are outputs.  2 <= C <= PS_PCT_MAX_CHANNELS. */
int ps_gate_forward_f32(const float *vg, const float *u, int B, int C, int L, float *out, float *mean, float *rstd, void *stream);

/* Its backward pass writes the gradient of the whole (B,2C,H,W) operand; the gradient of u is dout itself and is not written.
 * With s = sigmoid(g), vh = (v - mean) * rstd recomputed, a = dout * s (fp32):
 *   m1 = sum a / C,  m2 = sum a * vh / (C - 1)   (fp64, rounded once);   dv = rstd * ((a - m1) - vh * m2);   dg = (dout * vh) * (s * (1 - s)) */
int ps_gate_backward_f32(const float *vg, const float *dout, const float *mean, const float *rstd, int B, int C, int L, float *dvg,
                         void *stream);

/* The backward pass of the mean cross entropy of given codes over the locations of a group.  logits, layout, targets, region,
 * temperature, F and L as ps_code_nll_f32 takes them (include/pixelsynth_nll.h: layout 0 = (F,512,L), 1 = (F,L,512) aligned to 16
 * bytes); frames (F,2,4) fp64 is what that call left; groups = PS_PCT_GROUP_OBSERVED | PS_PCT_GROUP_SAMPLED or one of them;
 * grad_out one fp32 value on the device.  count = the sum over the frames of the chosen groups' counts (integers: exact),
 *   scale = fp32(double(grad_out) / count / temperature)
 *   grad[f,c,l] = scale * (softmax(logits / T)[c] - [c == target])      for a location of a chosen group
 *               = +0.0                                                  elsewhere
 * written in the logits' own layout.  The softmax is exp((x - M) / T) / s, M the row's largest logit, s the fp32 sum of the 512
 * exponentials (layout 0: a wavefront adds its 128 classes as eight chains of 16 joined as a tree, then the four wavefronts as a tree;
 * layout 1: a lane its 8 classes as a tree, then a butterfly over the lanes) and the quotient a true division.  A location of a chosen
 * group with a target outside [0, 512) or a NaN logit gets a row of NaN, as the forward gives it a NaN. */
int ps_code_nll_backward_f32(const float *logits, int layout, const int32_t *targets, const uint8_t *region, const double *frames,
                             int groups, double temperature, int F, int L, const float *grad_out, float *grad_logits, void *stream);

/* ps_pixelcnn_train_last_error: the message of this library's last failed call. */
const char *ps_pixelcnn_train_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_PIXELCNN_TRAIN_H */
