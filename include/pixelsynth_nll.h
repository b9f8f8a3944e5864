/* pixelsynth_nll.h -- the C ABI of libpixelsynth_nll.so: the likelihood the PixelCNN gives to GIVEN codes (csrc/code_nll.hip) -- per
 * location the negative log-likelihood of the target code, the entropy of the predicted distribution and whether the target is the
 * arg-max, and per frame their fp64 sums over the observed and the sampled locations.  A library of its own beside
 * libpixelsynth_hip.so, whose pinned set of exports it leaves as it is.  Same conventions: int status, 0 = success,
 * ps_nll_last_error() says why not; every buffer is the caller's; the last parameter is the stream; no allocation, no synchronisation,
 * no device-to-host copy, no atomics.  Every result is bit-identical from run to run. */
#ifndef PIXELSYNTH_NLL_H
#define PIXELSYNTH_NLL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_NLL_CLASSES 512       /* classes of the logits */
#define PS_NLL_LAYOUT_CHW 0      /* logits (F,512,L), class-major: what ps_pixelcnn_forward_f32 writes */
#define PS_NLL_LAYOUT_LC 1       /* logits (F,L,512), by location: out_logits of the AR runs; 16-byte aligned */
#define PS_NLL_MAX_FRAMES 65535

/* logits fp32 in `layout`; targets (F,L) int32; region (F,L) uint8 by location, nonzero = sampled, 0 = observed (the convention of
 * the AR runs' sample region), or NULL: every location observed; temperature > 0; 1 <= F <= PS_NLL_MAX_FRAMES, L >= 1.
 * Per location (F,L), each NULL or written in full:
 *   nll      fp32, nats: logsumexp(x / T) - x_t / T.  The maximum is taken out before the exponentials; the exponentials and their sum
 *            are fp32, the logarithm of the sum, the target's own term and the difference fp64, rounded once.  A NaN logit gives NaN; a
 *            target outside [0, 512) is never used as an index and gives NaN.
 *   entropy  fp32, nats: -sum p log p of softmax(x / T); a class whose exponential underflows to 0 contributes 0.
 *   hit      uint8: 1 where the target is the arg-max of the logits, the lowest class among equal maxima; 0 for a target outside
 *            [0, 512).
 * Per frame: frames (F,2,4) fp64 or NULL, [f][g] = {count, sum nll, sum entropy, sum hit} over the locations of group g (0 observed,
 * 1 sampled) -- the fp64 sums of the three per-location outputs, which it therefore needs (all three non-NULL): one workgroup per
 * frame, thread t takes locations t, t + 256, ... in that order, then a fixed pairwise tree; a frame's row depends on nothing but
 * the frame, and is the same bits alone as at any position of a batch.  An empty group: count 0, sums 0.
 * Layout 0 runs one workgroup per 64 consecutive locations, lanes across the locations, its four waves a quarter of the classes each;
 * layout 1 one wave per location, eight consecutive classes per lane. */
int ps_code_nll_f32(const float *logits, int layout, const int32_t *targets, const uint8_t *region, double temperature, int F, int L,
                    float *nll, float *entropy, uint8_t *hit, double *frames, void *stream);

/* ps_nll_last_error: the message of this library's last failed call. */
const char *ps_nll_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_NLL_H */
