// splat.hip -- depth un-projection + camera transform + soft z-buffer splat for gfx950 (MI355X).
//
// Replaces, behind the C ABI of include/pixelsynth_hip.h:
//   PtsManipulator.project_pts / project_pts_cumulative   models/projection/z_buffer_manipulator.py:50-83, 221-266
//   RasterizePointsXYsBlending.forward                    models/layers/z_buffer_layers.py:55-131
//   + PyTorch3D rasterize_points / compositing it calls   (third party, semantics in DESIGN.md section 2)
//
// Pipeline (all on the caller's stream, no host sync, no allocation):
//   k_project        1 thread / point: p = grid*depth, X = K (RT2 RT1inv) Kinv p, divide, EPS rule
//   splat_core       bin, sort per tile, composite, dilate: csrc/splat_pipeline.h (its kernels are listed there), which
//                    csrc/scene.hip includes as well
//
// Integer/index paths are bit-exact against oracle/ (this file is built with -ffp-contract=off: the
// disc test dx*dx+dy*dy < r*r and the z ordering must not be perturbed by FMA contraction).  What the projection shares with the other
// units of the family (mat4_vec, the camera prologue, the grid point, finish_point) is csrc/splat_math.h's.  The hard z-buffer of
// DepthManipulator and ps_read_status are csrc/zbuffer.hip.
#include "splat_pipeline.h"

namespace {

// grid-stride clear of `count` words by a 2-D grid of 256-thread workgroups
__device__ __forceinline__ void clear_words(uint32_t *__restrict__ words, unsigned count)
{
    for (unsigned i = (blockIdx.y * gridDim.x + blockIdx.x) * 256u + threadIdx.x; i < count; i += gridDim.x * gridDim.y * 256u)
        words[i] = 0u;
}

// LAYOUT 0: sampler (B,3,NT) as the reference returns it; LAYOUT 1: (B,NT,3) with x,y negated, i.e.
// exactly what PyTorch3D's rasterizer is handed after z_buffer_layers.py:71-72.
// PRIOR: the source is a homogeneous prior cloud (B,4,n) transformed by K (RT2 RT3inv)  (:244-247).
template <int LAYOUT, bool PRIOR>
__global__ __launch_bounds__(256) void k_project(const float *__restrict__ src,
                                                 const int32_t *__restrict__ new_index,
                                                 const float *__restrict__ K,
                                                 const float *__restrict__ Kinv __attribute__((nonnull)),
                                                 const float *__restrict__ RTa_inv,
                                                 const float *__restrict__ RT2, int W, int n,
                                                 int out_n, int out_off, float *__restrict__ out,
                                                 float *__restrict__ cloud, uint32_t *__restrict__ zero_words = nullptr,
                                                 unsigned zero_count = 0)
{
    __shared__ float sRT[16], sK[16], sKinv[16];
    const int b = blockIdx.y;
    // (the fused project + splat call: the binning counters of the splat that follows are cleared here, not by a memset of their own)
    clear_words(zero_words, zero_count);
    load_cams(K, PRIOR ? nullptr : Kinv, RTa_inv, RT2, b, sRT, sK, sKinv);
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    float X[4];
    if (PRIOR) {
        float p[4], w[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = src[((size_t)b * 4 + r) * n + t];
        mat4_vec(sRT, p, w);
        mat4_vec(sK, w, X);
    } else {
        const int g = new_index ? new_index[(size_t)b * n + t] : t;
        float p[4], c[4], w[4];
        GridPixel(g, W).point(src[(size_t)b * n + t], p);
        mat4_vec(sKinv, p, c);
        mat4_vec(sRT, c, w);
        mat4_vec(sK, w, X);
    }
    float sx, sy, sz;
    finish_point(X, sx, sy, sz);
    const int o = out_off + t;
    if (LAYOUT == 0) {
        out[((size_t)b * 3 + 0) * out_n + o] = sx;
        out[((size_t)b * 3 + 1) * out_n + o] = sy;
        out[((size_t)b * 3 + 2) * out_n + o] = sz;
    } else {
        float *q = out + ((size_t)b * out_n + o) * 3;
        q[0] = -sx;
        q[1] = -sy;
        q[2] = sz;
    }
    if (cloud) {
#pragma unroll
        for (int r = 0; r < 4; ++r) cloud[((size_t)b * 4 + r) * out_n + o] = X[r];
    }
}

// z_buffer_layers.py:71-72 -- the reference negates x,y of the caller's tensor in place
__global__ void k_negate_xy(float *pts, size_t npts)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npts) return;
    pts[i * 3 + 1] = -pts[i * 3 + 1];
    pts[i * 3 + 0] = -pts[i * 3 + 0];
}

}  // namespace

extern "C" {

size_t ps_splat_workspace_bytes(int B, int N, int S, double radius_px)
{
    if (B <= 0 || N <= 0 || S <= 1 || radius_px <= 0) return 0;
    return make_plan(B, N, S, radius_px).total;
}

int ps_project_pts_f32(const float *depth, const float *K, const float *Kinv, const float *RT1inv,
                       const float *RT2, int B, int W, float *sampler, void *stream)
{
    PS_REQUIRE(depth && K && Kinv && RT1inv && RT2 && sampler, "project_pts: null pointer");
    PS_REQUIRE(B > 0 && W > 1, "project_pts: B > 0 and W > 1 required");
    const int N = W * W;
    hipLaunchKernelGGL((k_project<0, false>), dim3((N + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, depth,
                       (const int32_t *)nullptr, K, Kinv, RT1inv, RT2, W, N, N, 0, sampler, (float *)nullptr);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_project_pts_cumulative_f32(const float *depth_new, const int32_t *new_index, const float *prior,
                                  const float *K, const float *Kinv, const float *RT1inv, const float *RT2,
                                  const float *RT3inv, int B, int W, int n_new, int n_prior, float *sampler,
                                  float *cloud, void *stream)
{
    PS_REQUIRE(K && Kinv && RT1inv && RT2 && sampler && cloud, "project_pts_cumulative: null pointer");
    PS_REQUIRE(B > 0 && W > 1 && n_new >= 0 && n_prior >= 0 && n_new + n_prior > 0, "project_pts_cumulative: bad sizes");
    PS_REQUIRE(new_index || n_new == W * W || n_new == 0, "project_pts_cumulative: n_new != W*W needs new_index");
    PS_REQUIRE(n_prior == 0 || (prior && RT3inv), "project_pts_cumulative: prior cloud needs RT3inv");
    const int NTt = n_new + n_prior;
    hipStream_t st = (hipStream_t)stream;
    if (n_new > 0) {
        PS_REQUIRE(depth_new, "project_pts_cumulative: depth_new is null");
        hipLaunchKernelGGL((k_project<0, false>), dim3((n_new + 255) / 256, B), dim3(256), 0, st, depth_new, new_index,
                           K, Kinv, RT1inv, RT2, W, n_new, NTt, 0, sampler, cloud);
    }
    if (n_prior > 0)
        hipLaunchKernelGGL((k_project<0, true>), dim3((n_prior + 255) / 256, B), dim3(256), 0, st, prior,
                           (const int32_t *)nullptr, K, Kinv, RT3inv, RT2, W, n_prior, NTt, n_new, sampler, cloud);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_splat_f32(float *pts, const float *feat, int B, int N, int C, int S, double radius_px, int K, float tau,
                 int rad_pow, int accumulation, int bg_ksize, float *out_feat, uint8_t *out_bg, int32_t *out_idx,
                 float *out_zbuf, float *out_dist, void *workspace, size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(pts && feat && out_feat && out_bg && workspace, "splat: null pointer");
    if (int rc = check_splat_args(B, N, C, S, radius_px, K, accumulation, bg_ksize)) return rc;
    const SplatPlan p = make_plan(B, N, S, radius_px);
    if (workspace_bytes < p.total)
        return ps::fail(PS_ERR_WORKSPACE, "splat: workspace %zu < required %zu bytes", workspace_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    const size_t npts = (size_t)B * N;
    hipLaunchKernelGGL(k_negate_xy, dim3((unsigned)((npts + 255) / 256)), dim3(256), 0, st, pts, npts);
    return splat_core(pts, feat, B, N, C, S, radius_px, K, tau, rad_pow, accumulation, bg_ksize, out_feat, out_bg,
                      out_idx, out_zbuf, out_dist, (char *)workspace, p, st);
}

int ps_project_splat_f32(const float *depth, const float *feat, const float *K, const float *Kinv,
                         const float *RT1inv, const float *RT2, int B, int C, int S, double radius_px, int Kpp,
                         float tau, int rad_pow, int accumulation, int bg_ksize, float *out_feat, uint8_t *out_bg,
                         void *workspace, size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(depth && feat && K && Kinv && RT1inv && RT2 && out_feat && out_bg && workspace,
               "project_splat: null pointer");
    const int N = S * S;
    if (int rc = check_splat_args(B, N, C, S, radius_px, Kpp, accumulation, bg_ksize)) return rc;
    const SplatPlan p = make_plan(B, N, S, radius_px);
    if (workspace_bytes < p.total)
        return ps::fail(PS_ERR_WORKSPACE, "project_splat: workspace %zu < required %zu bytes", workspace_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    float *pts = (float *)((char *)workspace + p.off_pts);
    hipLaunchKernelGGL((k_project<1, false>), dim3((N + 255) / 256, B), dim3(256), 0, st, depth,
                       (const int32_t *)nullptr, K, Kinv, RT1inv, RT2, S, N, N, 0, pts, (float *)nullptr,
                       (uint32_t *)((char *)workspace + p.off_count), (unsigned)((p.off_bg0 - p.off_count) / sizeof(uint32_t)));
    return splat_core(pts, feat, B, N, C, S, radius_px, Kpp, tau, rad_pow, accumulation, bg_ksize, out_feat, out_bg,
                      nullptr, nullptr, nullptr, (char *)workspace, p, st, true);
}

}  // extern "C"
