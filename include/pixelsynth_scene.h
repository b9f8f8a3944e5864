/* pixelsynth_scene.h -- the C ABI of libpixelsynth_scene.so: one frame of B independent chained trajectories
 * (ZbufferModelPts.forward_scene, model settings gen_scene / gen_two_imgs) per call, over accumulated point clouds of DIFFERENT lengths
 * (csrc/scene.hip, which builds on the kernels of csrc/splat_pipeline.h, the ones csrc/splat.hip launches).  A library of its own next to libpixelsynth_hip.so, whose ABI (version 2)
 * it leaves as it is.  Same conventions as include/pixelsynth_hip.h: int status, 0 = success, ps_scene_last_error() says why not; every
 * buffer is the caller's; the last parameter is the stream; no allocation, no synchronisation, no device-to-host copy.
 *
 * Replaces PtsManipulator.forward_justpts_cumulative / project_pts_cumulative (models/projection/z_buffer_manipulator.py:184-266) and
 * the splat they feed (models/layers/z_buffer_layers.py:55-131) for a batch of scenes.
 *
 * STATE, caller-owned, per scene b of B, for at most `cap` points (fixed when the state is created):
 *   cloud   two buffers (B,4,cap) f32   the homogeneous points in the camera of the last rendered frame (with the EPS write of :253-254);
 *                                       a step reads one in full and writes the other in full -- every prior point is re-projected by
 *                                       K (RT2 RT3inv) each frame (:244-247), so the ping-pong pair costs no traffic a single buffer would save
 *   feat    two buffers (B,C,cap) f32   the points' features, ping-pong like the cloud: a step moves the prior features behind the new ones
 *                                       (C/4 of the cloud's traffic), and the composite reads them by plain point index, as it always did
 *   count   (B) int32                   points scene b holds; entries [count[b], cap) of its rows are undefined
 *   ORDER RULE: logical point i of scene b is column i of its rows.  A step puts the frame's NEW points first, in row-major order of
 *   last_bg, then the PRIOR cloud in its existing order (:248-266, :199-206).  The rasterizer breaks z ties by point index, so this order
 *   is what makes scene b of a batch the B = 1 route's result bit for bit.
 *   Footprint per scene: ps_scene_state_bytes(1, C, cap) = (2 * 4 + 2 * C) * 4 * cap + 4 bytes
 *   (C = 3, cap = 3 * 256^2: 11.0 MB).
 * WORKSPACE per scene: the splat's for a cloud of cap points -- 12 cap (points) + 4 cap (bounding boxes) + 8 T cap (keys, T = tiles a
 *   disc can touch: 9 at radius 4) + 16 ceil(S/8)^2 + S^2 (tile tables, undilated mask) -- plus 4 (ceil(S^2/256) + 1) for the compaction's
 *   block sums, each part rounded up to 256 bytes: ps_scene_workspace_bytes(1, cap, S, radius_px)  (cap = 3 * 256^2, S = 256, radius 4: 17.4 MB).
 *   Both queries are host-only arithmetic and return 0 for a non-positive size. */
#ifndef PIXELSYNTH_SCENE_H
#define PIXELSYNTH_SCENE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t ps_scene_state_bytes(int B, int C, int cap);
size_t ps_scene_workspace_bytes(int B, int cap, int S, double radius_px);

/* One frame of every scene.
 *   depth (B,1,S,S) f32, feat_new (B,C,S,S) f32: the frame each scene is rendered FROM (its depth and features per pixel).
 *   last_bg (B,S,S) uint8 (bool): background mask of the previously rendered frame -- pixel t of scene b becomes a new point iff
 *     last_bg[b,t] != 0; its slot is its rank among the set pixels in row-major order (an exclusive scan, never an atomic).
 *     NULL: the first frame of a chain -- no prior, every pixel is a point (S*S per scene, exactly PtsManipulator.forward_justpts),
 *     count is overwritten; cloud_prev, feat_prev, RT3inv are unused and prior_max must be 0.
 *   cloud_prev / feat_prev: the state's current buffers (read), cloud_next / feat_next: the other pair (written); count: read, then
 *     updated in place to the new counts.  The caller swaps the pairs after the call.
 *   K, Kinv, RT1inv, RT2, RT3inv (B,4,4) f32: new points by K (RT2 RT1inv) Kinv, prior points by K (RT2 RT3inv).
 *   prior_max, next_max: the largest count over the scenes before and after this step.  The host knows every count exactly (the popcount
 *     of the mask it has already read back for the AR plan, plus the previous count); they size the launches.  next_max > cap is refused
 *     before anything is enqueued; independently the kernels never index past cap.  Nothing is ever dropped silently.
 *   radius_px ... bg_ksize: as ps_splat_f32.  out_feat (B,C,S,S) f32, out_bg (B,S,S) uint8: as ps_project_splat_f32 (the product route).
 *   workspace: >= ps_scene_workspace_bytes(B, cap, S, radius_px) bytes of device memory. */
int ps_scene_step_f32(const float *depth, const float *feat_new, const uint8_t *last_bg, const float *cloud_prev,
                      const float *feat_prev, float *cloud_next, float *feat_next, int32_t *count, const float *K,
                      const float *Kinv, const float *RT1inv, const float *RT2, const float *RT3inv, int B, int C, int S, int cap,
                      int prior_max, int next_max, double radius_px, int Kpp, float tau, int rad_pow, int accumulation, int bg_ksize,
                      float *out_feat, uint8_t *out_bg, void *workspace, size_t workspace_bytes, void *stream);

/* ps_scene_last_error: the message of this library's last failed call. */
const char *ps_scene_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_SCENE_H */
