// splat_math.h -- the arithmetic the splat family shares, defined once: csrc/splat.hip (projection), csrc/splat_pipeline.h (binning,
// sort, composite), csrc/scene.hip (the chained-scene step), csrc/splat_bwd.hip (the backward passes), csrc/zbuffer.hip (the hard
// z-buffer) and tools/sqrt_probe.hip.  These units must agree bit for bit on the projection of a point, on the box a point is binned
// into and on the disc test, so each of them is written here and nowhere else.  Every fp32 expression keeps its association order; the
// units that include this header are built with -ffp-contract=off.
#pragma once
#include <cmath>

#include "ps_common.h"

namespace {

constexpr int TILE = 8;                  // pixels per tile edge: 64 pixels = one wave64
constexpr float PS_EPS = 1e-2f;          // z_buffer_manipulator.py:8
constexpr uint32_t CULLED = 0xFFFFFFFFu;
constexpr float D_LO = 1e-3f;            // the clamp of dist^2 / denom to [D_LO, 1] (z_buffer_layers.py:89-91)
constexpr float T_MIN = 1e-4f;           // the floor of wsumnorm's denominator (PyTorch3D's kEpsilon)

// ------------------------------------------------------------------------------------------
// projection
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void mat4_vec(const float *M, const float *v, float *o)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float acc = M[i * 4 + 0] * v[0];
        acc = acc + M[i * 4 + 1] * v[1];
        acc = acc + M[i * 4 + 2] * v[2];
        acc = acc + M[i * 4 + 3] * v[3];
        o[i] = acc;
    }
}

// RT = A B of image b's (4,4) poses (mul, add, ascending k), K and -- unless Kinv is null -- Kinv into LDS: the prologue of every kernel
// that projects; ends in a barrier.  A literal nullptr folds the test away; a kernel whose Kinv the host never lets be null declares
// the parameter nonnull, which folds it too.  (No __restrict__ here: inlined, its scopes move the callers' instructions.)
__device__ __forceinline__ void load_cams(const float *K, const float *Kinv, const float *RTa_inv, const float *RT2, int b, float *sRT,
                                          float *sK, float *sKinv)
{
    if (threadIdx.x < 16) {
        const int i = threadIdx.x >> 2, j = threadIdx.x & 3;
        const float *A = RT2 + b * 16, *Bm = RTa_inv + b * 16;
        float acc = A[i * 4 + 0] * Bm[0 * 4 + j];
        acc = acc + A[i * 4 + 1] * Bm[1 * 4 + j];
        acc = acc + A[i * 4 + 2] * Bm[2 * 4 + j];
        acc = acc + A[i * 4 + 3] * Bm[3 * 4 + j];
        sRT[threadIdx.x] = acc;
        sK[threadIdx.x] = K[b * 16 + threadIdx.x];
        if (Kinv) sKinv[threadIdx.x] = Kinv[b * 16 + threadIdx.x];
    }
    __syncthreads();
}

// pixel g (row-major) of the W x W grid: its align-corners coordinates linspace(0,W-1,W)/(W-1)*2-1  (:38-39), and from them the
// homogeneous point at depth d, p = (xs d, -ys d, -d, 1), and the derivative of p with respect to d
struct GridPixel {
    float xs, ys;
    __device__ __forceinline__ GridPixel(int g, int W)
    {
        const int gx = g % W, gy = g / W;
        const float den = (float)(W - 1);
        xs = (float)gx / den * 2.0f - 1.0f;
        ys = (float)gy / den * 2.0f - 1.0f;
    }
    __device__ __forceinline__ void point(float d, float *p) const { p[0] = xs * d; p[1] = (-ys) * d; p[2] = -1.0f * d; p[3] = 1.0f; }
    __device__ __forceinline__ void d_point(float *dp) const { dp[0] = xs; dp[1] = -ys; dp[2] = -1.0f; dp[3] = 0.0f; }
};

// sampler of one projected homogeneous point; X[2] is EPS-overwritten like the reference (:70-74)
__device__ __forceinline__ void finish_point(float *X, float &sx, float &sy, float &sz)
{
    const bool bad = fabsf(X[2]) < PS_EPS;
    if (bad) X[2] = PS_EPS;
    float x = X[0] / (-X[2]);
    float y = X[1] / (-X[2]);
    float z = X[2];
    if (bad) { x = -10.0f; y = -10.0f; z = -10.0f; }
    sx = x * 1.0f;
    sy = y * -1.0f;
    sz = z * -1.0f;
}

// ------------------------------------------------------------------------------------------
// binning
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float pix_to_ndc(int i, int S) { return -1.0f + (2 * i + 1.0f) / S; }

// Conservative range of pixel indices whose centre can pass the strict disc test, per axis.
// PyTorch3D tests output pixel xi against PixToNdc(S-1-xi); c is the point in reversed-index units.
__device__ __forceinline__ bool axis_range(float p, int S, float hw, int &lo_px, int &hi_px)
{
    const float c = ((p + 1.0f) * S - 1.0f) * 0.5f;
    float lo = c - hw, hi = c + hw;
    if (!(hi >= 0.0f) || !(lo <= (float)(S - 1))) return false;  // also rejects NaN / inf
    lo = fmaxf(lo, 0.0f);
    hi = fminf(hi, (float)(S - 1));
    const int ilo = (int)ceilf(lo), ihi = (int)floorf(hi);
    if (ilo > ihi) return false;
    lo_px = S - 1 - ihi;
    hi_px = S - 1 - ilo;
    return true;
}

__device__ __forceinline__ uint32_t point_bbox(const float *p, int S, float hw)
{
    const float px = p[0], py = p[1], pz = p[2];
    if (!(pz >= 0.0f)) return CULLED;  // PyTorch3D skips pz < 0; NaN z is skipped too (documented)
    int x0, x1, y0, y1;
    if (!axis_range(px, S, hw, x0, x1) || !axis_range(py, S, hw, y0, y1)) return CULLED;
    return (uint32_t)(x0 / TILE) | ((uint32_t)(y0 / TILE) << 8) | ((uint32_t)(x1 / TILE) << 16) |
           ((uint32_t)(y1 / TILE) << 24);
}

// ------------------------------------------------------------------------------------------
// the hit of a pixel
// ------------------------------------------------------------------------------------------
// Correctly rounded square root of d in [1e-3, 1] (the clamped dist^2 / r^2 of a hit): the hardware's 1-ulp v_sqrt_f32 and the check of
// its two neighbours that sqrtf itself expands to -- without sqrtf's rescaling of inputs below 2^-96 and its pass-through of 0 / inf,
// 7 of its 16 instructions, in a loop body of ~46.  Equal to sqrtf bit for bit on the whole range (tools/sqrt_probe.hip checks
// every float in [2^-20, 2]).
__device__ __forceinline__ float sqrt_rn_unit(float x)
{
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sm = __uint_as_float(__float_as_uint(s) - 1u), sp = __uint_as_float(__float_as_uint(s) + 1u);
    const float em = __builtin_fmaf(-sm, s, x), ep = __builtin_fmaf(-sp, s, x);
    float r = em <= 0.0f ? sm : s;
    r = ep > 0.0f ? sp : r;
    return r;
}

__device__ __forceinline__ float bcast(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// ------------------------------------------------------------------------------------------
// host: what a call derives from (S, radius_px, rad_pow), in the precisions the reference computes it in -- python double first, then
// float at the PyTorch3D call.  The forward, its workspace plan and the backward all take these from here.
// ------------------------------------------------------------------------------------------
struct SplatGeom {
    double radius;       // in NDC units                                      z_buffer_layers.py:77
    float rf, r2;        // the disc test's dx*dx + dy*dy < r2
    float denom;         // radius^rad_pow                                    :89
    bool pow2;           // denom is a power of two: then d2 / denom == d2 * (1 / denom) exactly
    float denom_arg;     // what k_composite is handed: 1 / denom if pow2, else denom
    float hw;            // conservative half-width, in pixels, of the box a point is binned into
    int tilesX;          // tiles per image row
    int max_tiles_pp;    // tiles one point's box can touch

    SplatGeom(int S, double radius_px, int rad_pow = 2)   // (hw, tilesX and max_tiles_pp do not depend on rad_pow)
    {
        radius = radius_px / (double)S * 2.0;
        rf = (float)radius;
        r2 = rf * rf;
        denom = (float)pow(radius, (double)rad_pow);
        int e = 0;
        pow2 = std::frexp(denom, &e) == 0.5f;
        denom_arg = pow2 ? 1.0f / denom : denom;
        hw = (float)(radius_px * 1.0001 + 0.01);
        tilesX = (S + TILE - 1) / TILE;
        const int span_px = (int)(2.0 * hw) + 2;
        const int span_t = (span_px + TILE - 2) / TILE + 1;
        max_tiles_pp = span_t * span_t;
    }
};

}  // namespace
