/* pixelsynth_content.h -- the C ABI of libpixelsynth_content.so: what lies between the convolutions of the VGG19 content loss of the
 * reference's SynthesisLoss (models/losses/synthesis.py:85-104, models/networks/architectures.py:52-85), forward and backward
 * (csrc/content_loss.hip).  A library of its own beside libpixelsynth_hip.so, whose pinned set of exports it leaves as it is; the
 * thirteen convolutions, their gradient scaling and the 64 -> 3 gradient to the image are that library's and
 * libpixelsynth_conv_bwd.so's exports.  Same conventions: int status, 0 = success, ps_content_last_error() says why not; every buffer
 * and the workspace are the caller's; the last parameter is the stream; one launch per call, no allocation, no synchronisation, no
 * device-to-host copy, no atomics.  Every result is bit-identical from run to run, on every card.
 *
 * Layout: NHWC fp32, C a multiple of 64, every buffer aligned to 16 bytes.  A pass holds P pairs as 2P images: prediction i is image i,
 * its target image P + i (PercSim's order).  Maps are PRE-ReLU outputs of a convolution; the ReLU is applied where a map is read.
 *
 * The loss:  L_l = mean |relu(y_l[pred]) - relu(y_l[gt])| over the P C Hl Wl elements of the tapped map l (conv1_1, conv2_1, conv3_1,
 * conv4_1, conv5_1), the batch mean nn.L1Loss takes;  total = sum_l w_l L_l,  w = (1/32, 1/16, 1/8, 1/4, 1).
 *
 * conv1_1's bias: ps_conv3x3_thin_in_f16x3_nhwc adds none.  It is ADDED ONCE, in place, by ps_content_bias on conv1_1's output, so the
 * tap, the join's mask, the next convolution (a plain ReLU as its act) and the saved map all see y + b; no other entry point here
 * takes a bias. */
#ifndef PIXELSYNTH_CONTENT_H
#define PIXELSYNTH_CONTENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_CONTENT_LEVELS 5
/* A tile of the tap: this many consecutive pixels of the prediction's images, numbered n = (i Hl + y) Wl + x over the P images (a tile
 * may span two images; the last one may be short).  tiles = ceil(P Hl Wl / PS_CONTENT_TILE).  Inside a tile, its float4 elements
 * e = (n - first n) C / 4 + c4 are dealt to PS_CONTENT_THREADS threads, thread t taking e = t, t + PS_CONTENT_THREADS, ... in ascending
 * order; a thread adds the four channels of an element in ascending order to ONE fp64 chain; the threads' sums are joined by the fixed
 * tree s[t] += s[t + h], h = PS_CONTENT_THREADS / 2, ..., 1. */
#define PS_CONTENT_TILE 256
#define PS_CONTENT_THREADS 256

/* ceil(npix / PS_CONTENT_TILE): the doubles a tap over npix = P Hl Wl prediction pixels writes. */
size_t ps_content_tiles(size_t npix);

/* The input pass: pred, gt (P, 3, H, W) fp32, read in place through element strides (int64[4]: batch, channel, row, column; none
 * negative) -> out (2P, H, W, 4), image i from pred[i], image P + i from gt[i], channel 3 zero.  No value is changed.
 * 1 <= P <= 32767. */
int ps_content_input(const float *pred, const int64_t *strides_pred, const float *gt, const int64_t *strides_gt, int P, int H, int W,
                     float *out, void *stream);

/* y[p][c] += bias[c] in place, y (npix, C): conv1_1's bias (above). */
int ps_content_bias(float *y, const float *bias, size_t npix, int C, void *stream);

/* The tap of a map y (2P, Hl, Wl, C): sums[t] = the fp64 sum over tile t (above) of |relu(y[i]) - relu(y[P + i])|, both operands
 * converted to fp64 before the subtraction, so the only error is that of the fp64 summation.  Writes ps_content_tiles(P Hl Wl)
 * doubles and nothing else.  relu keeps a NaN (and +inf); a NaN or inf - inf makes its tile's sum NaN. */
int ps_content_tap(const float *y, int P, int Hl, int Wl, int C, double *sums, void *stream);

/* The finish: sums holds the five levels' tiles one block after the other, tiles[l] doubles for level l (host array of
 * PS_CONTENT_LEVELS); counts[l] = P C Hl Wl of level l (host array).  Per level the tiles are added in ascending order (one fp64
 * chain), levels[l] = fp32(sum_l / counts[l]); total[0] = fp32(sum_l w_l (sum_l / counts[l])), formed in fp64 in ascending l and
 * rounded once.  A level with tiles[l] = 0 gives levels[l] = 0 and adds nothing to the total. */
int ps_content_finish(const double *sums, const int64_t *tiles, const int64_t *counts, float *levels, float *total, void *stream);

/* pooled (N, Hl / 2, Wl / 2, C) = the 2 x 2 stride-2 max-pool of the pre-ReLU map y (N, Hl, Wl, C), Hl and Wl even.  The ReLU
 * commutes with it (the next convolution applies it on the way in).  A window that holds a NaN gives NaN, as F.max_pool2d does. */
int ps_content_pool(const float *y, int N, int Hl, int Wl, int C, float *pooled, void *stream);

/* The backward join, the one pass between two grad_input convolutions.  For the prediction's map y (P, Hl, Wl, C) it writes
 *     G = [not (y <= 0)] * (route(up) * inv_s + c * sign(relu(y) - relu(y_gt)))                      (P, Hl, Wl, C)
 * the gradient at the convolution's output (torch's threshold_backward: a NaN in y lets the gradient through; where y <= 0 the result
 * is an exact 0 whatever the bracket holds).
 *   up: the output of the consumer's grad_input convolution, still multiplied by its scale s; inv_s = scale2[1] (scale2 = {s, 1 / s}
 *     on the device, as ps_conv3x3_bwd_prepare_f32 leaves it).  up = NULL (conv5_1): no first term, scale2 is not read.
 *   pooled = 0: up is (P, Hl, Wl, C), route is the identity.  pooled != 0: a 2 x 2 max-pool lies between, up is (P, Hl / 2, Wl / 2,
 *     C), and each of its elements goes to the one element of its window torch's max_pool2d picks -- the window scanned (0,0), (0,1),
 *     (1,0), (1,1), a strictly greater value replaces, a NaN always replaces --, the other three get 0.  (Picked on y, not relu(y): the
 *     picks differ only among values <= 0, which the mask zeroes.)
 *   y_gt (P, Hl, Wl, C): the target's map of a tapped level, or NULL: no second term (g and weight are not read).
 *     c = (g[0] * weight) / fp32(count), fp32 products and a true fp32 division, count = P C Hl Wl (exact in fp32 for the network's
 *     sizes); g: the loss's incoming gradient, one float on the device; weight = w_l.  relu keeps a NaN; sign(0) = sign(NaN) = 0 as
 *     torch.sign; both terms are rounded to fp32 before they are added (no contraction).
 * G must not overlap an input. */
int ps_content_join(const float *y, const float *y_gt, const float *up, const float *scale2, const float *g, float weight, int P, int Hl,
                    int Wl, int C, int pooled, float *G, void *stream);

/* ps_content_last_error: the message of this library's last failed call. */
const char *ps_content_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_CONTENT_H */
