// splat_bwd.hip -- the backward pass of the soft z-buffer splat and of the reprojection for gfx950 (MI355X), behind the C ABI of
// include/pixelsynth_splat_bwd.h (the formulas are stated there).
//
// In the reference the splat is PyTorch3D's differentiable renderer: rasterize_points' backward (the squared distance of a hit with
// respect to the point's x and y; z only ever receives grad_zbuf, which the compositing does not produce), compositing.*'s backward
// (alphas and features), and autograd through project_pts (models/projection/z_buffer_manipulator.py:50-83).  Here:
//   k_splat_bwd_pixels   1 lane / pixel, 8 x 8 tiles as k_composite: reads the pixel's saved K-nearest list (idx, dist) and grad_out
//                        for ALL channels (q_k = <g, f_{n_k}> needs every one, so channel groups are not split over the grid), walks
//                        front to back for a_k, cum_k, q_k and back to front for the recurrence R; writes the per-hit coefficients
//                        w[p,k] and gd2[p,k] = dL/dd2 into the workspace (the two planes are its scratch on the way).
//   k_splat_bwd_points   1 wave / point, a GATHER: walks the pixels of the point's conservative box (axis_range of splat_math.h,
//                        the one the forward bins with) in row-major order, 64 pixels a round, one per lane; a lane runs the forward's exact
//                        disc test and looks for the point's packed index among the K entries of its pixel.  Features: lane c owns
//                        channel c and adds the round's hits in lane (= row-major pixel) order.  Coordinates: every lane adds its own
//                        pixels round by round, then a fixed xor butterfly.  No atomics anywhere: two runs give the same bits, and a
//                        cloud's gradients do not depend on what else is in the batch.  A box of thousands of pixels (large radii)
//                        is walked the same way: correct, not fast.
//   k_project_bwd        1 thread / point: the projected point is affine in the depth, so the gradient is closed form.
// Built with -ffp-contract=off like splat.hip: the disc test and the distances must be the forward's, bit for bit -- the pixel and box
// arithmetic, the projection's helpers and the constants are csrc/splat_math.h's, the forward's own.
#include "splat_math.h"

#include "../../include/pixelsynth_splat_bwd.h"

namespace {

// alpha of a hit from its squared distance, as k_composite's list-emitting route computes it (sqrtf is correctly rounded, as its
// sqrt_rn_unit); root: sqrt(d); inside: the quotient lies strictly between the clamp bounds
__device__ __forceinline__ float alpha_of(float d2, float denom, float tau, float &root, bool &inside)
{
    const float r = d2 / denom;
    inside = r > D_LO && r < 1.0f;
    const float d = fminf(fmaxf(r, D_LO), 1.0f);
    root = sqrtf(d);
    float a = 1.0f - root;
    if (tau != 1.0f) a = powf(a, tau);
    return a;
}

// ------------------------------------------------------------------------------------------
// per pixel: the coefficients of every hit
// ------------------------------------------------------------------------------------------
constexpr int QCH = 8;   // channels of grad_out a lane keeps in registers while it walks its list once

template <int MODE>
__global__ __launch_bounds__(64) void k_splat_bwd_pixels(const int32_t *__restrict__ idx, const float *__restrict__ dist,
                                                         const float *__restrict__ feat, const float *__restrict__ grad_out, int N,
                                                         int C, int S, int tilesX, int K, float denom, float tau, int need_pts,
                                                         float *__restrict__ plane_w, float *__restrict__ plane_g)
{
    const int tile = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int xi = (tile % tilesX) * TILE + (lane & 7), yi = (tile / tilesX) * TILE + (lane >> 3);
    if (xi >= S || yi >= S) return;
    const size_t SS = (size_t)S * S;
    const size_t pix = (size_t)b * SS + (size_t)yi * S + xi;
    const int32_t *li = idx + pix * K;
    const float *ld = dist + pix * K;
    float *pw = plane_w + pix * K, *pg = plane_g + pix * K;
    const float *g = grad_out + (size_t)b * C * SS + (size_t)yi * S + xi;
    const float *fb = feat + (size_t)b * C * N;
    const int base = b * N;

    // front to back: alpha, transmittance; plane_w <- q_k (0 for now), plane_g <- cum_k (alphacomposite) or a_k
    float cum = 1.0f, tsum = 0.0f;
    int m = 0;
    for (; m < K; ++m) {
        const int v = li[m];
        if (v < base || v - base >= N) break;   // -1 behind the last hit (an index of another cloud ends the list too)
        float root;
        bool inside;
        const float a = alpha_of(ld[m], denom, tau, root, inside);
        pw[m] = 0.0f;
        pg[m] = MODE == PS_ACC_ALPHACOMPOSITE ? cum : a;
        cum = cum * (1.0f - a);
        tsum = tsum + a;
    }
    if (need_pts) {
        for (int c0 = 0; c0 < C; c0 += QCH) {
            float gv[QCH];
#pragma unroll
            for (int j = 0; j < QCH; ++j) gv[j] = c0 + j < C ? g[(size_t)(c0 + j) * SS] : 0.0f;
            for (int k = 0; k < m; ++k) {
                const float *f = fb + (size_t)c0 * N + (li[k] - base);
                float q = pw[k];
#pragma unroll
                for (int j = 0; j < QCH; ++j)
                    if (c0 + j < C) q = q + gv[j] * f[(size_t)j * N];
                pw[k] = q;
            }
        }
    }
    const float T = fmaxf(tsum, T_MIN);
    float wq = 0.0f;                             // wsumnorm: sum_t w_t q_t
    if (MODE == PS_ACC_WSUMNORM && need_pts) {
        for (int k = 0; k < m; ++k) wq = wq + pg[k] / T * pw[k];
    }
    // back to front: R, the weights and dL/dd2
    float R = 0.0f;
    for (int k = m - 1; k >= 0; --k) {
        const float q = pw[k], c1 = pg[k];
        float root;
        bool inside;
        const float a0 = alpha_of(ld[k], denom, tau, root, inside);
        float w, dLda;
        if (MODE == PS_ACC_ALPHACOMPOSITE) {
            w = c1 * a0;
            dLda = c1 * (q - R);
            R = a0 * q + (1.0f - a0) * R;
        } else if (MODE == PS_ACC_WSUM) {
            w = c1;
            dLda = q;
        } else {
            w = c1 / T;
            dLda = tsum >= T_MIN ? (q - wq) / T : q / T;
        }
        const float om = 1.0f - root;
        if (tau < 1.0f && !(om > 0.0f)) inside = false;
        float pwr = 1.0f;
        if (tau != 1.0f) pwr = powf(om, tau - 1.0f);
        const float dadd2 = -tau * pwr / (2.0f * root * denom);
        pw[k] = w;
        pg[k] = inside ? dLda * dadd2 : 0.0f;    // a select: the clamp's derivative is exactly 0, whatever the other factor
    }
}

// ------------------------------------------------------------------------------------------
// per point: gather over the pixels of its box
// ------------------------------------------------------------------------------------------
constexpr int PWAVES = 4;   // points (waves) per workgroup; the waves never synchronise

__global__ __launch_bounds__(64 * PWAVES) void k_splat_bwd_points(const float *__restrict__ pts, const int32_t *__restrict__ idx,
                                                                  const float *__restrict__ plane_w, const float *__restrict__ plane_g,
                                                                  const float *__restrict__ grad_out, int N, int C, int S, int K,
                                                                  float hw, float r2, float *__restrict__ grad_pts,
                                                                  float *__restrict__ grad_feat)
{
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int n = blockIdx.x * PWAVES + (threadIdx.x >> 6);
    if (n >= N) return;                                   // (wave-uniform)
    const size_t SS = (size_t)S * S;
    const float *p = pts + ((size_t)b * N + n) * 3;
    const float px = p[0], py = p[1], pz = p[2];
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    const bool live = (pz >= 0.0f) && axis_range(px, S, hw, x0, x1) && axis_range(py, S, hw, y0, y1);
    const int bw = x1 - x0 + 1;
    const int npx = live ? bw * (y1 - y0 + 1) : 0;
    const int packed = b * N + n;
    const float *gb = grad_out + (size_t)b * C * SS;

    for (int c0 = 0; c0 < (grad_feat ? C : 1); c0 += 64) {    // (more than 64 channels: the box is walked once per 64)
        const int c = c0 + lane;
        const bool do_pts = c0 == 0 && grad_pts;
        float acc = 0.0f, accx = 0.0f, accy = 0.0f;
        for (int i0 = 0; i0 < npx; i0 += 64) {
            const int i = i0 + lane;
            bool found = false;
            float w = 0.0f, gx = 0.0f, gy = 0.0f;
            int poff = 0;
            if (i < npx) {
                const int yy = y0 + i / bw, xx = x0 + i % bw;
                const float xf = pix_to_ndc(S - 1 - xx, S), yf = pix_to_ndc(S - 1 - yy, S);
                const float dx = px - xf, dy = py - yf;
                const float d2 = dx * dx + dy * dy;
                if (d2 < r2) {                           // the forward's strict disc test: only these pixels can list the point
                    poff = yy * S + xx;
                    const size_t e = ((size_t)b * SS + poff) * K;
                    for (int k = 0; k < K; ++k) {
                        const int v = idx[e + k];
                        if (v < 0) break;
                        if (v == packed) {
                            found = true;
                            w = plane_w[e + k];
                            const float gd = plane_g[e + k];
                            gx = gd * (2.0f * dx) * -1.0f;   // d d2 / d px, and the negation the forward applied
                            gy = gd * (2.0f * dy) * -1.0f;
                            break;
                        }
                    }
                }
            }
            if (do_pts) {
                accx = accx + gx;
                accy = accy + gy;
            }
            if (grad_feat) {
                unsigned long long hits = __ballot(found);
                while (hits) {                           // (wave-uniform) the round's hits in row-major pixel order
                    const int j = __builtin_ctzll(hits);
                    hits &= hits - 1;
                    const float wj = bcast(w, j);
                    const int pj = __builtin_amdgcn_readlane(poff, j);
                    if (c < C) acc = acc + wj * gb[(size_t)c * SS + pj];
                }
            }
        }
        if (grad_feat && c < C) grad_feat[((size_t)b * C + c) * N + n] = acc;
        if (do_pts) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                accx = accx + __shfl_xor(accx, off, 64);
                accy = accy + __shfl_xor(accy, off, 64);
            }
            if (lane < 3) grad_pts[((size_t)b * N + n) * 3 + lane] = lane == 0 ? accx : lane == 1 ? accy : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------
// projection (the backward of splat.hip's k_project)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_project_bwd(const float *__restrict__ depth, const float *__restrict__ K,
                                                     const float *__restrict__ Kinv __attribute__((nonnull)), const float *__restrict__ RT1inv,
                                                     const float *__restrict__ RT2, const float *__restrict__ grad_sampler, int W, int n,
                                                     float *__restrict__ grad_depth)
{
    __shared__ float sRT[16], sK[16], sKinv[16];
    const int b = blockIdx.y;
    load_cams(K, Kinv, RT1inv, RT2, b, sRT, sK, sKinv);
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    float p[4], dp[4], c[4], w[4], X[4], m1[4];
    const GridPixel g(t, W);
    g.point(depth[(size_t)b * n + t], p);                      // the forward's point
    g.d_point(dp);                                             // its derivative with respect to the depth
    mat4_vec(sKinv, p, c);
    mat4_vec(sRT, c, w);
    mat4_vec(sK, w, X);
    mat4_vec(sKinv, dp, c);
    mat4_vec(sRT, c, w);
    mat4_vec(sK, w, m1);
    const float g0 = grad_sampler[((size_t)b * 3 + 0) * n + t], g1 = grad_sampler[((size_t)b * 3 + 1) * n + t],
                g2 = grad_sampler[((size_t)b * 3 + 2) * n + t];
    const float z2 = X[2] * X[2];
    const float dsx = -(m1[0] * X[2] - X[0] * m1[2]) / z2;     // sampler x = -X0 / X2
    const float dsy = (m1[1] * X[2] - X[1] * m1[2]) / z2;      // sampler y =  X1 / X2
    const float dsz = -m1[2];                                  // sampler z = -X2
    const float gd = g0 * dsx + g1 * dsy + g2 * dsz;
    grad_depth[(size_t)b * n + t] = fabsf(X[2]) < PS_EPS ? 0.0f : gd;   // the constant -10 has no derivative
}

size_t plane_bytes(int B, int S, int K) { return ps::align_up((size_t)B * S * S * K * sizeof(float), 256); }

bool sizes_ok(int B, int S, int K) { return B > 0 && B <= 65535 && S > 1 && S <= 2048 && K > 0; }

}  // namespace

extern "C" {

const char *ps_splat_bwd_last_error(void) { return ps::last_error_ref().c_str(); }

size_t ps_splat_bwd_workspace_bytes(int B, int S, int K)
{
    if (!sizes_ok(B, S, K)) return 0;
    return 2 * plane_bytes(B, S, K);
}

int ps_splat_backward_f32(const float *pts_negated, const float *feat, const int32_t *idx, const float *dist, const float *grad_out,
                          int B, int N, int C, int S, double radius_px, int K, float tau, int rad_pow, int accumulation,
                          float *grad_pts, float *grad_feat, void *workspace, size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(grad_pts || grad_feat, "splat_backward: no output (grad_pts and grad_feat are both NULL)");
    PS_REQUIRE(pts_negated && feat && idx && dist && grad_out && workspace, "splat_backward: null pointer");
    PS_REQUIRE(sizes_ok(B, S, K) && N > 0 && C > 0, "splat_backward: B = %d, N = %d, C = %d, S = %d, K = %d: expected B in [1, 65535], "
               "N, C, K >= 1 and S in [2, 2048]", B, N, C, S, K);
    PS_REQUIRE(radius_px > 0 && radius_px <= 64, "splat_backward: radius_px %.3f out of range (0,64]", radius_px);
    PS_REQUIRE(accumulation >= 0 && accumulation <= 2, "splat_backward: unknown accumulation %d", accumulation);
    PS_REQUIRE((size_t)B * N < 0x7FFFFFFFull, "splat_backward: B*N overflows the packed int32 index");
    const size_t need = 2 * plane_bytes(B, S, K);
    if (workspace_bytes < need)
        return ps::fail(PS_ERR_WORKSPACE, "splat_backward: workspace %zu < required %zu bytes", workspace_bytes, need);
    PS_REQUIRE((uintptr_t)workspace % 4 == 0, "splat_backward: the workspace must be aligned to 4 bytes");
    hipStream_t st = (hipStream_t)stream;
    float *plane_w = (float *)workspace, *plane_g = (float *)((char *)workspace + plane_bytes(B, S, K));
    const SplatGeom geom(S, radius_px, rad_pow);               // the forward's radius, denominator and box (splat_core takes them from here too)
    const float r2 = geom.r2, denom = geom.denom, hw = geom.hw;
    const int tilesX = geom.tilesX;
    const dim3 gp(tilesX * tilesX, B);
    const int need_pts = grad_pts != nullptr;
#define PS_BWD_PIXELS(MODE)                                                                                                     \
    hipLaunchKernelGGL(k_splat_bwd_pixels<MODE>, gp, dim3(64), 0, st, idx, dist, feat, grad_out, N, C, S, tilesX, K, denom, tau, \
                       need_pts, plane_w, plane_g)
    switch (accumulation) {
    case PS_ACC_ALPHACOMPOSITE: PS_BWD_PIXELS(PS_ACC_ALPHACOMPOSITE); break;
    case PS_ACC_WSUM: PS_BWD_PIXELS(PS_ACC_WSUM); break;
    default: PS_BWD_PIXELS(PS_ACC_WSUMNORM); break;
    }
#undef PS_BWD_PIXELS
    hipLaunchKernelGGL(k_splat_bwd_points, dim3((N + PWAVES - 1) / PWAVES, B), dim3(64 * PWAVES), 0, st, pts_negated, idx, plane_w, plane_g,
                       grad_out, N, C, S, K, hw, r2, grad_pts, grad_feat);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_project_pts_backward_f32(const float *depth, const float *K, const float *Kinv, const float *RT1inv, const float *RT2,
                                const float *grad_sampler, int B, int W, float *grad_depth, void *stream)
{
    PS_REQUIRE(depth && K && Kinv && RT1inv && RT2 && grad_sampler && grad_depth, "project_pts_backward: null pointer");
    PS_REQUIRE(B > 0 && B <= 65535 && W > 1 && W <= 16384, "project_pts_backward: B in [1, 65535] and W in [2, 16384] required");
    const int N = W * W;
    hipLaunchKernelGGL(k_project_bwd, dim3((N + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, depth, K, Kinv, RT1inv, RT2,
                       grad_sampler, W, N, grad_depth);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
