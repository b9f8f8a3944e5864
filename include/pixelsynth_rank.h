/* pixelsynth_rank.h -- the C ABI of libpixelsynth_rank.so: scoring and ranking the best-of-N candidates of a view on the device
 * (csrc/rank.hip).  A library of its own next to libpixelsynth_hip.so, whose ABI (version 2) it leaves as it is.  Same conventions as
 * include/pixelsynth_hip.h: int status, 0 = success, ps_rank_last_error() says why not; every buffer is the caller's; the last parameter
 * is the stream; no allocation, no synchronisation, no device-to-host copy, no atomics.  Every result is bit-identical from run to run
 * and does not depend on a candidate's place in its batch.
 *
 * The four passes stand for what the reference does per candidate on the host (models/z_buffermodel.py:254-276): the classifier's input
 * (reinterpretation, quantisation, Pillow's bilinear resize, normalisation), the entropy of its softmax, the fake side of the
 * discriminator's hinge loss, and the rank rule.  The two networks between them are the caller's. */
#ifndef PIXELSYNTH_RANK_H
#define PIXELSYNTH_RANK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_RANK_MAX_SIDE 1024   /* S and T of ps_rank_classifier_input */
#define PS_RANK_MAX_N 1024      /* n of ps_rank_select */

/* Candidates to classifier inputs, queued on `stream`; every pointer is a device pointer.
 *   imgs (N,3,S,S) fp32, nominally in [-1,1].  The 3*S*S floats of a candidate are READ AS an (S,S,3) interleaved image (the
 *     reference's reshape, not a permute) and quantised: u8 = trunc(((x * 0.5) + 0.5) * 255), every operation rounded to fp32, none
 *     fused.  Definition outside [-1,1]: the product is clamped to [-2^31, 2^31 - 128], truncated to int32, and its low byte taken; a
 *     NaN gives 0.
 *   bounds (T,2) int32, coeffs (T,ksize) int32: the tables of Pillow's BILINEAR resample of S to T samples -- for output index i the
 *     first input index and the number of taps, and the taps' weights in 22-bit fixed point (pixelsynth_amd.ranking.pil_bilinear_tables
 *     makes them).  The image is square, the same tables serve both passes: the horizontal one into uint8 -- (2^21 + sum p*k) >> 22
 *     clipped to 0..255 -- then the vertical one in the same way.  A bound outside the image is clipped to it (no read outside imgs).
 *   norm (3,256) fp32: norm[c][u] = the classifier's input for byte u of channel c (the host forms ((u/255 - mean_c)/std_c) in fp32).
 *   out (N,3,T,T) fp32: planar, out[n][c][y][x] = norm[c][resized[n][y][x][c]].
 *   bytes (N,T,T,3) uint8 or NULL: the resized image itself.
 * One workgroup per (candidate, band of output rows).  A null imgs, bounds, coeffs, norm or out, N <= 0, S or T outside
 * 1..PS_RANK_MAX_SIDE, ksize < 1: a nonzero status and a message, nothing is launched. */
int ps_rank_classifier_input(const float *imgs, int N, int S, int T, const int32_t *bounds, const int32_t *coeffs, int ksize,
                             const float *norm, float *out, uint8_t *bytes, void *stream);

/* entropy (N) fp32 of logits (N,n_classes) fp32: -sum p log p of the fp32 softmax with the row maximum subtracted.  One wave per row,
 * a fixed reduction tree.  A class whose probability underflows to 0 contributes 0 * log 0 = NaN (as numpy's probs * log(probs)). */
int ps_rank_entropy(const float *logits, int N, int n_classes, float *entropy, void *stream);

/* d_fake (N) fp32 from the last patch maps of the two discriminator scales, map0 (N,len0) and map1 (N,len1) fp32 (len = h * w):
 * d_fake[n] = (mean0 + mean1) / 2 with mean = -mean(min(-x - 1, 0)) over the candidate's map -- the hinge loss of the fake side, per
 * scale, then the mean over scales.  -x - 1 is rounded to fp32, the sums are carried in fp64 and rounded once.  One wave per candidate. */
int ps_rank_hinge_fake(const float *map0, int len0, const float *map1, int len1, int N, float *d_fake, void *stream);

/* The rank rule on disc (n) and entr (n) fp32, 1 <= n <= PS_RANK_MAX_N.  The rank of an element is the number of elements that sort
 * before it: ascending by value, the lower index first among equal values, NaN after every number.  total2 = (n - 1 - entr_rank) +
 * disc_rank; best[0] (int32) = the first index of its maximum.  disc_rank, entr_rank (n) int32 or NULL.  One workgroup.  The same rule
 * for every view of a batch, one workgroup per view, and the winners' hand-over: include/pixelsynth_rank_groups.h. */
int ps_rank_select(const float *disc, const float *entr, int n, int32_t *best, int32_t *disc_rank, int32_t *entr_rank, void *stream);

/* ps_rank_last_error: the message of this library's last failed call. */
const char *ps_rank_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_RANK_H */
