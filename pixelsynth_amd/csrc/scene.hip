// scene.hip -- one frame of B independent chained trajectories (ZbufferModelPts.forward_scene) in one pass, for gfx950 (MI355X).
//
// Replaces, behind the C ABI of include/pixelsynth_scene.h (libpixelsynth_scene.so, a library of its own beside libpixelsynth_hip.so):
//   PtsManipulator.forward_justpts_cumulative   models/projection/z_buffer_manipulator.py:184-219   (a5)
//   PtsManipulator.project_pts_cumulative       models/projection/z_buffer_manipulator.py:221-266   (a4)
//   RasterizePointsXYsBlending.forward          models/layers/z_buffer_layers.py:55-131             (a6)
// for a batch whose scenes have accumulated clouds of DIFFERENT lengths.  The reference (and the B = 1 route of this repository) selects a
// frame's new points with boolean gathers and a view(bs, 1, -1), which needs equal counts per image and a device-to-host round trip per
// gather; here the selection is an ordered compaction on the device and the splat runs with per-cloud counts.
//
// The kernels of the splat and their host core are csrc/splat_pipeline.h, which csrc/splat.hip includes as well: k_bin_count / k_bin_fill
// with per-cloud counts, k_scan, k_sort_*, k_composite and k_dilate* as they are -- one source, no second composite.
//
// Pipeline of ps_scene_step_f32 (all on the caller's stream, no host sync, no allocation):
//   k_scene_count   per scene and block of 256 pixels: how many pixels of last_background_mask are set
//   k_scan          exclusive scan of each scene's block sums (splat_pipeline.h's scan, key slice 0): the block's first output slot and,
//                   behind the last block, the scene's number of new points.  A scan, never an atomic: slot = rank in row-major order.
//   k_scene_prior   every prior point t of scene b: X = K (RT2 RT3inv) p (:244-247) -> slot n_new[b] + t of the next cloud, its features
//                   moved along
//   k_scene_new     every kept pixel: p = grid * depth, X = K (RT2 RT1inv) Kinv p (:229-243) -> slot rank of the next cloud, its features
//                   from the frame; block (0, b) then publishes count[b] += n_new[b]
//   splat_core      with counts: the points at or past count[b] do not exist
// The arithmetic of a point is k_project's (the helpers of csrc/splat_math.h, -ffp-contract=off), and a point's slot is the index
// the B = 1 route gives it (new points first in row-major order of the mask, then the prior cloud in its order, :248-266): the
// rasterizer breaks z ties by point index, so the results are the B = 1 route's bit for bit.
#include "splat_pipeline.h"

#include "../../include/pixelsynth_scene.h"

namespace {

constexpr int SB = 256;   // pixels per block of the compaction

// a projected point into slot o (< cap, checked by the caller) of scene b: the homogeneous cloud (B,4,cap) and the rasterizer's
// (B,cap,3) with x, y negated (what z_buffer_layers.py:71-72 hands PyTorch3D)
__device__ __forceinline__ void scene_store(float *X, int b, int o, int cap, float *__restrict__ cloud, float *__restrict__ pts)
{
    float sx, sy, sz;
    finish_point(X, sx, sy, sz);
    float *q = pts + ((size_t)b * cap + o) * 3;
    q[0] = -sx;
    q[1] = -sy;
    q[2] = sz;
#pragma unroll
    for (int r = 0; r < 4; ++r) cloud[((size_t)b * 4 + r) * cap + o] = X[r];
}

__global__ __launch_bounds__(SB) void k_scene_count(const uint8_t *__restrict__ mask, int N, int nblk, uint32_t *__restrict__ blk)
{
    const int b = blockIdx.y, t = blockIdx.x * SB + threadIdx.x;
    const int c = __syncthreads_count(t < N && mask[(size_t)b * N + t] != 0);
    if (threadIdx.x == 0) blk[(size_t)b * (nblk + 1) + blockIdx.x] = (uint32_t)c;
}

// mask == nullptr: the first frame -- every pixel is a new point, slot = pixel, no block sums
__global__ __launch_bounds__(SB) void k_scene_new(const float *__restrict__ depth, const float *__restrict__ feat_new,
                                                  const uint8_t *__restrict__ mask, const uint32_t *__restrict__ blk,
                                                  const float *__restrict__ K, const float *__restrict__ Kinv,
                                                  const float *__restrict__ RT1inv, const float *__restrict__ RT2, int W, int C,
                                                  int nblk, int cap, float *__restrict__ cloud, float *__restrict__ feat,
                                                  float *__restrict__ pts, int32_t *__restrict__ count)
{
    __shared__ float sRT[16], sK[16], sKinv[16];
    __shared__ uint32_t wave_n[SB / 64];
    const int b = blockIdx.y, N = W * W;
    load_cams(K, Kinv, RT1inv, RT2, b, sRT, sK, sKinv);
    const int t = blockIdx.x * SB + threadIdx.x;
    const bool keep = t < N && (!mask || mask[(size_t)b * N + t] != 0);
    // rank of a kept pixel inside the block, in thread (= row-major) order
    const unsigned long long bal = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t o = mask ? blk[(size_t)b * (nblk + 1) + blockIdx.x] : (uint32_t)blockIdx.x * SB;
    for (int w = 0; w < wave; ++w) o += wave_n[w];
    o += (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // (k_scene_prior, which reads the old count, ran before this kernel)
        const long long n = mask ? (long long)count[b] + blk[(size_t)b * (nblk + 1) + nblk] : (long long)N;   // (a first frame starts the chain over)
        count[b] = (int32_t)(n < cap ? n : cap);   // (the host refused a step that does not fit; the clamp keeps a misuse inside the rows)
    }
    if (!keep || o >= (uint32_t)cap) return;
    float p[4], c[4], w[4], X[4];
    GridPixel(t, W).point(depth[(size_t)b * N + t], p);
    mat4_vec(sKinv, p, c);
    mat4_vec(sRT, c, w);
    mat4_vec(sK, w, X);
    scene_store(X, b, (int)o, cap, cloud, pts);
    for (int ch = 0; ch < C; ++ch) feat[((size_t)b * C + ch) * cap + o] = feat_new[((size_t)b * C + ch) * N + t];
}

__global__ __launch_bounds__(SB) void k_scene_prior(const float *__restrict__ cloud_prev, const float *__restrict__ feat_prev,
                                                    const uint32_t *__restrict__ blk, const int32_t *__restrict__ count,
                                                    const float *__restrict__ K, const float *__restrict__ RT3inv,
                                                    const float *__restrict__ RT2, int C, int nblk, int cap,
                                                    float *__restrict__ cloud, float *__restrict__ feat, float *__restrict__ pts)
{
    __shared__ float sRT[16], sK[16];
    const int b = blockIdx.y;
    load_cams(K, nullptr, RT3inv, RT2, b, sRT, sK, nullptr);
    const int t = blockIdx.x * SB + threadIdx.x;
    if (t >= min(count[b], cap)) return;
    const size_t o = (size_t)blk[(size_t)b * (nblk + 1) + nblk] + (size_t)t;   // behind the scene's new points
    if (o >= (size_t)cap) return;
    float p[4], w[4], X[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = cloud_prev[((size_t)b * 4 + r) * cap + t];
    mat4_vec(sRT, p, w);
    mat4_vec(sK, w, X);
    scene_store(X, b, (int)o, cap, cloud, pts);
    for (int ch = 0; ch < C; ++ch) feat[((size_t)b * C + ch) * cap + o] = feat_prev[((size_t)b * C + ch) * cap + t];
}

struct ScenePlan {
    SplatPlan splat;
    int nblk;
    size_t off_blk, total;
};

ScenePlan make_scene_plan(int B, int cap, int S, double radius_px)
{
    ScenePlan p;
    p.splat = make_plan(B, cap, S, radius_px);
    p.nblk = (S * S + SB - 1) / SB;
    p.off_blk = p.splat.total;
    p.total = ps::align_up(p.off_blk + (size_t)B * (p.nblk + 1) * sizeof(uint32_t), 256);
    return p;
}

}  // namespace

extern "C" {

const char *ps_scene_last_error(void) { return ps::last_error_ref().c_str(); }

size_t ps_scene_state_bytes(int B, int C, int cap)
{
    if (B <= 0 || C <= 0 || cap <= 0) return 0;
    return 2 * (size_t)B * 4 * cap * sizeof(float) + 2 * (size_t)B * C * cap * sizeof(float) + (size_t)B * sizeof(int32_t);
}

size_t ps_scene_workspace_bytes(int B, int cap, int S, double radius_px)
{
    if (B <= 0 || cap <= 0 || S <= 1 || radius_px <= 0) return 0;
    return make_scene_plan(B, cap, S, radius_px).total;
}

int ps_scene_step_f32(const float *depth, const float *feat_new, const uint8_t *last_bg, const float *cloud_prev,
                      const float *feat_prev, float *cloud_next, float *feat_next, int32_t *count, const float *K,
                      const float *Kinv, const float *RT1inv, const float *RT2, const float *RT3inv, int B, int C, int S, int cap,
                      int prior_max, int next_max, double radius_px, int Kpp, float tau, int rad_pow, int accumulation, int bg_ksize,
                      float *out_feat, uint8_t *out_bg, void *workspace, size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(depth && feat_new && cloud_next && feat_next && count && K && Kinv && RT1inv && RT2 && out_feat && out_bg && workspace,
               "scene_step: null pointer");
    PS_REQUIRE(cap > 0 && prior_max >= 0 && next_max > 0, "scene_step: cap, next_max must be > 0 and prior_max >= 0");
    if (int rc = check_splat_args(B, cap, C, S, radius_px, Kpp, accumulation, bg_ksize)) return rc;
    const int N = S * S;
    if (last_bg) {
        PS_REQUIRE(prior_max > 0 && cloud_prev && feat_prev && RT3inv, "scene_step: a chained frame needs the prior cloud, its features and RT3inv");
        PS_REQUIRE(cloud_prev != cloud_next && feat_prev != feat_next, "scene_step: the step is not in place (a ping-pong pair of buffers)");
    } else {
        PS_REQUIRE(prior_max == 0 && next_max == N, "scene_step: the first frame (no mask) has no prior and S*S points per scene");
    }
    PS_REQUIRE(next_max >= prior_max && next_max - prior_max <= N, "scene_step: next_max %d is not prior_max %d plus at most S*S", next_max, prior_max);
    if (next_max > cap)   // (the caller, who knows every scene's count, names the scene: this is the last line of defence)
        return ps::fail(PS_ERR_ARG, "scene_step: a scene would hold %d points, the state was created for cap = %d", next_max, cap);
    const ScenePlan p = make_scene_plan(B, cap, S, radius_px);
    if (workspace_bytes < p.total)
        return ps::fail(PS_ERR_WORKSPACE, "scene_step: workspace %zu < required %zu bytes", workspace_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    float *pts = (float *)(ws + p.splat.off_pts);
    uint32_t *blk = (uint32_t *)(ws + p.off_blk);
    const dim3 gnew(p.nblk, B);
    if (last_bg) {
        hipLaunchKernelGGL(k_scene_count, gnew, dim3(SB), 0, st, last_bg, N, p.nblk, blk);
        hipLaunchKernelGGL(k_scan, dim3(B), dim3(1024), 0, st, blk, p.nblk, 0u);
        hipLaunchKernelGGL(k_scene_prior, dim3((prior_max + SB - 1) / SB, B), dim3(SB), 0, st, cloud_prev, feat_prev, blk, count, K,
                           RT3inv, RT2, C, p.nblk, cap, cloud_next, feat_next, pts);
    }
    hipLaunchKernelGGL(k_scene_new, gnew, dim3(SB), 0, st, depth, feat_new, last_bg, blk, K, Kinv, RT1inv, RT2, S, C, p.nblk, cap,
                       cloud_next, feat_next, pts, count);
    return splat_core(pts, feat_next, B, cap, C, S, radius_px, Kpp, tau, rad_pow, accumulation, bg_ksize, out_feat, out_bg, nullptr,
                      nullptr, nullptr, ws, p.splat, st, false, count, next_max);
}

}  // extern "C"
