/* pixelsynth_plan.h -- the C ABI of libpixelsynth_plan.so: the generation orders of an AR plan worked out on the device, from
 * background masks that are already there (csrc/ar_order.hip).  A library of its own next to libpixelsynth_hip.so, whose ABI (version 2)
 * it leaves as it is.  Same conventions as include/pixelsynth_hip.h: int status, 0 = success, ps_plan_last_error() says why not; every
 * buffer is the caller's; the last parameter is the stream; no allocation, no synchronisation, no device-to-host copy.
 *
 * ps_plan_order gives, bit for bit, what ps_ar_plan (include/pixelsynth_hip.h) returns in order_loc and region, the first sampled rank
 * of every frame (ps_ar_plan reports their minimum as first_step) and every mask's number of set pixels: 8x8 pooling of the mask, two
 * 5x5 chamfer distance transforms in 16.16 fixed point, the signed distance and the greedy frontier walk of the reference's custom_idx
 * (models/z_buffermodel.py:641-701, models/lmconv/get_custom_order.pyx:4-124).  One workgroup of 256 threads and 10.5 KB of LDS per
 * frame, one launch. */
#ifndef PIXELSYNTH_PLAN_H
#define PIXELSYNTH_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 for the shapes ps_plan_order handles -- 1 <= G <= 32, S a multiple of G, G <= S <= 4096 -- and 0 for every other; host arithmetic. */
int ps_plan_order_takes(int S, int G);

/* The orders of B frames, queued on `stream`; every pointer is a device pointer.
 *   bg (B,S,S) uint8: the background masks, any nonzero byte is set.  Block (by,bx) of S/G x S/G pixels is background iff all of its
 *     bytes are set and foreground iff none is.  Masks at a 16-byte aligned address with S % 16 == 0 are read 16 bytes per lane.
 *   order_loc (B,L) int32, L = G*G: the location row*G + col by rank in the generation order.
 *   region (B,L) uint8: 1 where the whole block is background (the sampled region, by location).
 *   first_steps (B) int32 or NULL: the first rank whose location is in the region, L if the frame has none.
 *   bg_counts (B) int32 or NULL: the set pixels of the frame's mask.
 * A null bg, order_loc or region, B <= 0 or a shape ps_plan_order_takes refuses: a nonzero status and a message, nothing is launched. */
int ps_plan_order(const uint8_t *bg, int B, int S, int G, int32_t *order_loc, uint8_t *region, int32_t *first_steps,
                  int32_t *bg_counts, void *stream);

/* ps_plan_last_error: the message of this library's last failed call. */
const char *ps_plan_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_PLAN_H */
