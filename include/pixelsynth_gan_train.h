/* pixelsynth_gan_train.h -- the C ABI of libpixelsynth_gan_train.so: what touches an activation-sized tensor when the multiscale
 * discriminator trains, besides its 4 x 4 convolutions (csrc/gan_train.hip; the reference's models/networks/discriminators.py and
 * compute_generator_loss of models/losses/gan_loss.py) -- instance normalisation + LeakyReLU, forward and backward, and the
 * feature-matching L1 over the intermediate maps, forward and backward.
 * libpixelsynth_hip.so's pinned set of exports stays as it is.  Same conventions: int status, 0 = success,
 * ps_gan_train_last_error() says why not; every buffer and the workspace are the caller's; the last parameter is the stream; no
 * allocation, no synchronisation, no device-to-host copy, no atomics.  Every result is bit-identical from run to run, and the results
 * of a plane (of a map) are the same bits whether it is passed alone or in a batch.
 *
 * Every tensor is fp32, dense NCHW: what torch's convolutions hand over.  A plane is the HW values of one (sample, channel); plane
 * bases are only aligned to 4 bytes (HW is odd at the network's own sizes, 65^2 = 4225), and nothing here asks for more. */
#ifndef PIXELSYNTH_GAN_TRAIN_H
#define PIXELSYNTH_GAN_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Which form a plane of HW values takes, a function of HW alone:
 *   HW <= PS_GAN_TRAIN_WAVE_HW                a wavefront per plane, four planes per workgroup of 256 threads; lane l holds the values
 *                                             l, l + 64, ... in registers, 4 ceil(ceil(HW / 64) / 4) of them (4 .. 32);
 *   HW <= PS_GAN_TRAIN_RESIDENT_HW            a workgroup per plane, thread t holds t, t + 256, ... in registers,
 *                                             4 ceil(ceil(HW / 256) / 4) of them (12 .. 32);
 *   above                                     a workgroup per plane that streams it: a pass for the sums, a second one for the result.
 * In the first two forms the forward reads x once and writes y once, and the backward reads x and dy once and writes dx once.
 * RESIDENT_HW is chosen from sizes, not measured: the backward's two planes are then 64 KiB, 64 registers per thread at 256 threads.
 * WAVE_HW is the same count of registers at 64 lanes; it takes the network's 17^2 .. 34^2 planes, and 65^2 goes to a workgroup.
 * A thread adds its values in ascending order in fp64, the lanes of a wavefront are added as a butterfly (lane ^ 1, ^ 2, .. ^ 32), the
 * four wavefronts of a workgroup in ascending order. */
#define PS_GAN_TRAIN_WAVE_HW 2048
#define PS_GAN_TRAIN_RESIDENT_HW 8192

/* Instance normalisation (nn.InstanceNorm2d(affine=False)) + LeakyReLU of `planes` planes of HW values.  Per plane, in fp64,
 *   S1 = sum x,  S2 = sum x^2 (the square of an fp32 value is exact there),  mean = S1 / HW,  var = max(S2 / HW - mean^2, 0)
 * (the biased variance; NaN stays NaN), each rounded once to fp32; rstd = 1 / sqrt(var + eps), the sum in fp32, its reciprocal root
 * rounded once to fp32.  Then in fp32, every operation rounded on its own,
 *   v = (x - mean) * rstd,   y = v > 0 ? v : v * slope        (a NaN stays a NaN, and reaches no other plane).
 * mean and rstd (one per plane) are outputs: the backward pass takes them.  HW = 1 gives y = 0.
 * Sizes: planes, HW >= 1.  No form needs a workspace: it may be NULL. */
int ps_in_lrelu_forward_f32(const float *x, int planes, int HW, float eps, float slope, float *y, float *mean, float *rstd,
                            void *workspace, size_t workspace_bytes, void *stream);

/* Its backward pass.  v is recomputed from x, mean and rstd as the forward computes it (the same bits); y is not needed.
 *   g = v > 0 ? dy : dy * slope                                  (fp32)
 *   m1 = sum g / HW,  m2 = sum g * v / HW                        (products and sums in fp64, each rounded once to fp32)
 *   dx = rstd * ((g - m1) - v * m2)                              (fp32)
 * HW = 1 gives dx = 0. */
int ps_in_lrelu_backward_f32(const float *x, const float *dy, const float *mean, const float *rstd, int planes, int HW, float slope,
                             float *dx, void *workspace, size_t workspace_bytes, void *stream);

/* Feature matching over up to PS_GAN_TRAIN_MAX_MAPS maps in one launch.  maps, half_elems, weights (and grads) are HOST arrays of
 * n_maps entries; they travel in the kernels' arguments.  Map k holds 2 n_k values, n_k = half_elems[k]: the fake half, then the
 * real half ((2P, C, H, W) of a batch of P fakes followed by P reals).  A half is cut into tiles of PS_GAN_TRAIN_TILE values (the
 * last may be shorter).  Inside a tile thread t of 256 adds |d|, d = f - r in fp32, for the values t, t + 256, ... in fp64, lanes and
 * wavefronts as above; a finishing kernel adds a map's tiles in ascending order:
 *   S_k = sum |d|,   per_map[k] = fp32(S_k / n_k),   total = fp32(sum_k weights[k] * (S_k / n_k))     (fp64, ascending k)
 * per_map (n_maps) and total (1) are device buffers.  1 <= n_k < 2^40. */
#define PS_GAN_TRAIN_MAX_MAPS 16
#define PS_GAN_TRAIN_TILE 16384

/* Bytes of workspace ps_gan_feat_l1_f32 needs (device memory, aligned to 16 bytes): a double per tile; 0 for sizes it refuses. */
size_t ps_gan_feat_workspace_bytes(const long long *half_elems, int n_maps);

int ps_gan_feat_l1_f32(const float *const *maps, const long long *half_elems, const double *weights, int n_maps, float *per_map,
                       float *total, void *workspace, size_t workspace_bytes, void *stream);

/* Its backward pass: grad_total is one fp32 value on the device, s_k = fp32(double(grad_total) * weights[k] / n_k); the fake half of
 * grads[k] gets s_k * sgn(d), sgn(0) = 0 and sgn(NaN) = NaN (torch's L1Loss), the real half +0.0 (the reference detaches it). */
int ps_gan_feat_l1_backward_f32(const float *const *maps, const long long *half_elems, const double *weights, int n_maps,
                                const float *grad_total, float *const *grads, void *stream);

/* ps_gan_train_last_error: the message of this library's last failed call. */
const char *ps_gan_train_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_GAN_TRAIN_H */
