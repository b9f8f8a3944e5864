// train_glue.hip -- the full-resolution passes between the units of the generator's training step, for gfx950 (MI355X): the depth head
// behind the regressor (k_depth_*) and the blend of the reprojected features with the decoded codes, joined with the mask channel and
// written as the decoder's channels-last input (k_combine_*), each forward and backward.  Behind the C ABI of
// include/pixelsynth_train_glue.h (libpixelsynth_train_glue.so); the header states every formula and where it rounds.
//
// Every kernel is elementwise and bound by memory: a lane owns one pixel, neighbouring lanes read neighbouring addresses of the NCHW
// planes (and of the byte mask), and the channels-last side moves as one 16-byte access per lane.  No LDS, no barrier, no reduction:
// a pixel's bits depend on its operands alone.  The transcendental is expf and every quotient a true division, as in the other
// training units: the values feed a gradient.
#include "ps_common.h"

#include <cmath>

#include "../../include/pixelsynth_train_glue.h"

namespace {

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void k_combine_fwd(const float *__restrict__ gen, const float *__restrict__ gt,
                                                         const uint8_t *__restrict__ mask, int N, int L, float4 *__restrict__ out)
{
    const long long q = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (q >= N) return;
    const int p = (int)q, b = p / L, l = p % L;
    const float bg = mask[p] ? 1.0f : 0.0f, fg = 1.0f - bg;
    const size_t at = (size_t)b * 3 * L + l;
    float4 o;
    o.x = gen[at] * fg + gt[at] * bg;
    o.y = gen[at + L] * fg + gt[at + L] * bg;
    o.z = gen[at + 2 * (size_t)L] * fg + gt[at + 2 * (size_t)L] * bg;
    o.w = fg;
    out[p] = o;
}

__global__ __launch_bounds__(THREADS) void k_combine_bwd(const float4 *__restrict__ grad, const uint8_t *__restrict__ mask, int N, int L,
                                                         float *__restrict__ dgen)
{
    const long long q = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (q >= N) return;
    const int p = (int)q, b = p / L, l = p % L;
    const float fg = mask[p] ? 0.0f : 1.0f;
    const float4 g = grad[p];
    const size_t at = (size_t)b * 3 * L + l;
    dgen[at] = g.x * fg;
    dgen[at + L] = g.y * fg;
    dgen[at + 2 * (size_t)L] = g.z * fg;
}

__device__ __forceinline__ float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(THREADS) void k_depth_fwd(const float *__restrict__ raw, int mode, float range, float lo, long long N,
                                                       float *__restrict__ depth, float *__restrict__ pred)
{
    const long long q = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (q >= N) return;
    const float s = sigmoid(raw[q]);
    const float d = mode == PS_GLUE_DEPTH_INVERSE ? 1.0f / (s * 10.0f + 0.01f) : s * range + lo;
    depth[q] = d;
    pred[q] = d / 5.0f - 1.0f;
}

__global__ __launch_bounds__(THREADS) void k_depth_bwd(const float *__restrict__ raw, const float *__restrict__ grad, int mode, float range,
                                                       long long N, float *__restrict__ draw)
{
    const long long q = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (q >= N) return;
    const float s = sigmoid(raw[q]), t = s * (1.0f - s), g = grad[q];
    if (mode == PS_GLUE_DEPTH_INVERSE) {
        const float d = 1.0f / (s * 10.0f + 0.01f);
        draw[q] = -(((g * 10.0f) * t) * (d * d));
    } else {
        draw[q] = (g * range) * t;
    }
}

int check_image(const char *who, int B, int H, int W)
{
    PS_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: B = %d, H = %d, W = %d, expected >= 1", who, B, H, W);
    PS_REQUIRE((long long)B * H * W < (1ll << 31), "%s: B * H * W = %lld pixels, expected fewer than 2^31", who, (long long)B * H * W);
    return PS_OK;
}

int check_depth(const char *who, int mode, double min_z, double max_z, long long N)
{
    PS_REQUIRE(mode == PS_GLUE_DEPTH_RANGE || mode == PS_GLUE_DEPTH_INVERSE, "%s: mode = %d, expected 0 (range) or 1 (inverse)", who, mode);
    PS_REQUIRE(N >= 1 && N < (1ll << 31), "%s: N = %lld, expected 1 .. 2^31 - 1 (one lane per value, at most 2^23 workgroups)", who, N);
    PS_REQUIRE(mode != PS_GLUE_DEPTH_RANGE || (std::isfinite(min_z) && std::isfinite(max_z)), "%s: min_z = %g, max_z = %g, expected finite values",
               who, min_z, max_z);
    return PS_OK;
}

inline dim3 blocks(long long N) { return dim3((unsigned)((N + THREADS - 1) / THREADS)); }

}  // namespace

extern "C" {

const char *ps_train_glue_last_error(void) { return ps::last_error_ref().c_str(); }

int ps_combine_mask_nhwc_f32(const float *gen_fs, const float *input_gt, const uint8_t *background_mask, int B, int H, int W, float *out,
                             void *stream)
{
    PS_REQUIRE(gen_fs && input_gt && background_mask && out, "combine_mask_nhwc: null pointer");
    if (int rc = check_image("combine_mask_nhwc", B, H, W)) return rc;
    PS_REQUIRE(ps::aligned16(out), "combine_mask_nhwc: out must be aligned to 16 bytes");
    const int L = H * W, N = B * L;
    hipLaunchKernelGGL(k_combine_fwd, blocks(N), dim3(THREADS), 0, (hipStream_t)stream, gen_fs, input_gt, background_mask, N, L, (float4 *)out);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_combine_mask_nhwc_backward_f32(const float *grad_out, const uint8_t *background_mask, int B, int H, int W, float *grad_gen,
                                      void *stream)
{
    PS_REQUIRE(grad_out && background_mask && grad_gen, "combine_mask_nhwc backward: null pointer");
    if (int rc = check_image("combine_mask_nhwc backward", B, H, W)) return rc;
    PS_REQUIRE(ps::aligned16(grad_out), "combine_mask_nhwc backward: grad_out must be aligned to 16 bytes");
    const int L = H * W, N = B * L;
    hipLaunchKernelGGL(k_combine_bwd, blocks(N), dim3(THREADS), 0, (hipStream_t)stream, (const float4 *)grad_out, background_mask, N, L,
                       grad_gen);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_depth_head_forward_f32(const float *raw, int mode, double min_z, double max_z, long long N, float *depth, float *pred_img,
                              void *stream)
{
    PS_REQUIRE(raw && depth && pred_img, "depth_head forward: null pointer");
    if (int rc = check_depth("depth_head forward", mode, min_z, max_z, N)) return rc;
    hipLaunchKernelGGL(k_depth_fwd, blocks(N), dim3(THREADS), 0, (hipStream_t)stream, raw, mode, (float)(max_z - min_z), (float)min_z, N,
                       depth, pred_img);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_depth_head_backward_f32(const float *raw, const float *grad_depth, int mode, double min_z, double max_z, long long N,
                               float *grad_raw, void *stream)
{
    PS_REQUIRE(raw && grad_depth && grad_raw, "depth_head backward: null pointer");
    if (int rc = check_depth("depth_head backward", mode, min_z, max_z, N)) return rc;
    hipLaunchKernelGGL(k_depth_bwd, blocks(N), dim3(THREADS), 0, (hipStream_t)stream, raw, grad_depth, mode, (float)(max_z - min_z), N,
                       grad_raw);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
