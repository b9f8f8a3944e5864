/* pixelsynth_splat_bwd.h -- the C ABI of libpixelsynth_splat_bwd.so: the backward pass of the soft z-buffer splat and of the
 * reprojection (csrc/splat_bwd.hip; in the reference PyTorch3D's rasterize_points / compositing.* backward behind
 * models/layers/z_buffer_layers.py:55-131, and autograd through models/projection/z_buffer_manipulator.py:50-83).  A library of its
 * own beside libpixelsynth_hip.so, whose pinned set of exports it leaves as it is.  Same conventions: int status, 0 = success,
 * ps_splat_bwd_last_error() says why not; every buffer and the workspace are the caller's; the last parameter is the stream; no
 * allocation, no synchronisation, no device-to-host copy, no atomics.  Every result is bit-identical from run to run, and the gradients
 * of cloud b are the same bits whether it is run alone or in a batch.
 *
 * Notation.  Pixel p of frame b has the hit list n_0 .. n_{m-1} (m <= K) the list-emitting route of ps_splat_f32 wrote, in (z, index)
 * order: idx[b,p,k] = b*N + n_k (-1 behind the last hit), dist[b,p,k] = d2_k, the squared NDC distance to the negated point.
 *   d_k = clamp(d2_k / denom, 1e-3f, 1), denom = (float)pow(2 radius_px / S, rad_pow);   a_k = (1 - sqrt(d_k))^tau
 *   g = grad_out[b,:,p],  q_k = <g, feat[b,:,n_k]> over all C channels
 *   alphacomposite: w_k = cum_k a_k, cum_k = prod_{t<k} (1 - a_t);  R_m = 0, R_k = a_k q_k + (1 - a_k) R_{k+1};
 *                   dL/da_k = cum_k (q_k - R_{k+1})                         (no division by 1 - a_k)
 *   wsum:           w_k = a_k;  dL/da_k = q_k
 *   wsumnorm:       T = max(sum a, 1e-4f), w_k = a_k / T;  dL/da_k = (q_k - sum_t w_t q_t) / T where sum a >= 1e-4f, else q_k / T
 *   da_k/dd2_k = -tau (1 - sqrt d_k)^(tau-1) / (2 sqrt(d_k) denom) where 1e-3f < d2_k / denom < 1 STRICTLY (the quotient as fp32 rounds
 *                it), exactly 0 where the clamp holds -- a select, never a product with 0; for tau < 1 also 0 where the rounded root is 1
 *                (alpha is 0 there, as at the clamp). */
#ifndef PIXELSYNTH_SPLAT_BWD_H
#define PIXELSYNTH_SPLAT_BWD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace ps_splat_backward_f32 needs (device memory, 256-byte aligned): two planes of B*S*S*K floats, the per-hit
 * coefficients w and dL/dd2; 0 for sizes it refuses. */
size_t ps_splat_bwd_workspace_bytes(int B, int S, int K);

/* pts_negated (B,N,3): the points as ps_splat_f32 left them (x and y negated); feat (B,C,N); idx (B,S,S,K) int32 and dist (B,S,S,K):
 * out_idx / out_dist of that call; grad_out (B,C,S,S).  radius_px, K, tau, rad_pow, accumulation: that call's.
 *   grad_feat[b,c,n]  = sum over (p,k) with n_k = n of w_k g_c                                        (B,C,N)
 *   grad_pts[b,n,0]   = sum over (p,k) with n_k = n of dL/dd2_k * 2 (px - xf_p) * (-1), likewise y     (B,N,3)
 *   grad_pts[b,n,2]   = 0: the z order is piecewise constant
 * with (px, py) the negated point and (xf_p, yf_p) the NDC centre pixel p is tested against: the gradient with respect to the caller's
 * values BEFORE the negation.  Either output may be NULL (not both); each one asked for is the same bits as when both are.  Every
 * element of an output is written: exact zeros for points that are culled, hit no pixel or lie behind a pixel's K-th hit.
 * k_splat_bwd_pixels: one lane per pixel (8 x 8 tiles), front to back for a_k, cum_k, q_k, back to front for R; writes the two planes.
 * k_splat_bwd_points: one wave per point, a gather over the pixels of the point's conservative box (the forward's bounding-box
 * arithmetic, csrc/splat_math.h: one definition for both) in row-major order, 64 pixels a round; per channel the hits are added in that order, the two coordinates lane by lane in
 * that order and then through a fixed butterfly. */
int ps_splat_backward_f32(const float *pts_negated, const float *feat, const int32_t *idx, const float *dist, const float *grad_out,
                          int B, int N, int C, int S, double radius_px, int K, float tau, int rad_pow, int accumulation,
                          float *grad_pts, float *grad_feat, void *workspace, size_t workspace_bytes, void *stream);

/* The backward of ps_project_pts_f32: depth (B,1,W*W), cameras (B,4,4), grad_sampler (B,3,W*W) -> grad_depth (B,1,W*W).
 * The projected homogeneous point is affine in the depth, X(d) = d m1 + m0 with M = K (RT2 RT1inv) Kinv applied to (gx d, -gy d, -d, 1);
 * sampler = (-X0 / X2, X1 / X2, -X2), so
 *   grad_depth = gs0 * -(m1_0 X2 - X0 m1_2) / X2^2 + gs1 * (m1_1 X2 - X1 m1_2) / X2^2 - gs2 * m1_2,
 * exactly 0 where |X2| < 1e-2: the sampler is the constant -10 there.  No gradient for the cameras. */
int ps_project_pts_backward_f32(const float *depth, const float *K, const float *Kinv, const float *RT1inv, const float *RT2,
                                const float *grad_sampler, int B, int W, float *grad_depth, void *stream);

/* ps_splat_bwd_last_error: the message of this library's last failed call. */
const char *ps_splat_bwd_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_SPLAT_BWD_H */
