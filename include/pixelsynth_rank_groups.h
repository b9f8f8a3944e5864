/* pixelsynth_rank_groups.h -- the C ABI of libpixelsynth_rank_groups.so: best-of-N PER VIEW for a batch of views on the device
 * (csrc/rank_groups.hip) -- the rank rule applied to every view's own candidates, and the hand-over of every view's winner.  A library
 * of its own beside libpixelsynth_rank.so, whose set of exports it leaves as it is; the rank rule is that library's own device code
 * (csrc/rank_select.h), compiled into both.  Same conventions as include/pixelsynth_rank.h: int status, 0 = success,
 * ps_rank_groups_last_error() says why not; every buffer is the caller's; the last parameter is the stream; no allocation, no
 * synchronisation, no device-to-host copy, no atomics.  Every result is bit-identical from run to run.
 *
 * A "group" is a view, its n "candidates" the outpaintings of that view.  The two entry points address candidate i of group g at
 * g * group_stride + i * cand_stride, and take two layouts of the groups * n entries:
 *   candidate-major  (group_stride, cand_stride) = (1, groups): what ZbufferModelPts.get_best_sample stacks -- candidate 0 of every
 *                    view, then candidate 1 of every view, ...
 *   group-major      (group_stride, cand_stride) = (n, 1).
 * Any other pair of strides is refused with a message, and nothing is launched (with groups == 1 or n == 1 the two coincide in
 * what they address). */
#ifndef PIXELSYNTH_RANK_GROUPS_H
#define PIXELSYNTH_RANK_GROUPS_H

#include <stddef.h>
#include <stdint.h>

#include "pixelsynth_rank.h"    /* PS_RANK_MAX_N */

#ifdef __cplusplus
extern "C" {
#endif

#define PS_RANK_MAX_GROUPS 65535   /* groups of both entry points */

/* The rank rule of ps_rank_select in every group on its own.  disc, entr: groups * n fp32 scores, strides in elements.
 * 1 <= n <= PS_RANK_MAX_N, 1 <= groups <= PS_RANK_MAX_GROUPS.  Per group: the rank of an element is the number of the group's elements
 * that sort before it (ascending by value, the lower index first among equal values, NaN after every number); total2 = (n - 1 -
 * entr_rank) + disc_rank; best[g] (groups int32, contiguous) = the first index 0 .. n-1 of its maximum.  disc_rank, entr_rank: groups *
 * n int32 addressed as the scores are, or NULL.  One workgroup per group, its scores in LDS.  With groups == 1 the results are
 * ps_rank_select's. */
int ps_rank_select_groups(const float *disc, const float *entr, int groups, int n, long group_stride, long cand_stride, int32_t *best,
                          int32_t *disc_rank, int32_t *entr_rank, void *stream);

/* The winners' hand-over: out (groups, item_floats) fp32, out[g] = item g * group_stride + best[g] * cand_stride of src (groups * n
 * items of item_floats floats each; strides in items, the same two layouts).  best (groups int32) is read on the device and clamped to
 * 0 .. n-1: nothing is read outside src whatever it holds.  16-byte loads and stores where item_floats % 4 == 0 and src and out are
 * 16-byte aligned, scalar ones otherwise; nothing is written past out[groups * item_floats).  Grid (chunks of an item, groups). */
int ps_rank_take_groups(const float *src, const int32_t *best, int groups, int n, long group_stride, long cand_stride, long item_floats,
                        float *out, void *stream);

/* ps_rank_groups_last_error: the message of this library's last failed call. */
const char *ps_rank_groups_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_RANK_GROUPS_H */
