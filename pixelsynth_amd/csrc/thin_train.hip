// thin_train.hip -- the backward passes of the refinement decoder's thin convolutions (conv_thin.hip, conv1x1.hip: 4 -> 64 and 128 -> 3,
// 3 x 3 and 1 x 1) for gfx950 (MI355X), fp32 throughout, behind the C ABI of include/pixelsynth_thin_train.h
// (libpixelsynth_thin_train.so, beside libpixelsynth_hip.so whose set of exports it leaves as it is).
//
// Like their forward passes these are no matrix products worth the name: one side of the layer has Cw = 32 .. 256 channels, the other
// T <= 4, and each kernel makes one pass over the wide tensor.  Both give a thread four wide channels (16 bytes per access) and fp32 FMAs
// on the vector ALU, 9 T of them per wide float.
//   k_thin_expand       wide from thin: a thread owns four channels of four neighbouring pixels, so one ds_read_b128 of weights feeds
//                       16 FMAs, and a workgroup stages the weights once for eight rows.  The thin values it needs (3 rows of 6
//                       pixels) come straight from memory -- a thin map is 4 .. 16 bytes per pixel, a workgroup's share of it sits in
//                       the vector L1, and every lane of a pixel reads the same address.  Staging that halo in LDS was not built.
//   k_thin_grad_weight  the k k T x Cw sums over all pixels: a workgroup takes 32 wide channels (8 lanes) of one part of the pixels,
//                       its 32 groups of lanes take the part's pixels in turn, every thread keeps k k T float4 accumulators (27 for
//                       the 128 -> 3 layer: 162 registers, three waves per SIMD; 36 for 4 -> 64: 250, two), the groups are added
//                       through LDS in ascending order, and k_thin_sum_parts adds the parts.  The thin values again come through
//                       the L1: 9 T floats per pixel, shared by the eight lanes of the pixel; a pixel off the frame's border takes
//                       its taps without a test.  The bias sums -- sums of a gradient, whose terms cancel -- ride along in fp64
//                       (four adds per pixel beside 9 T x 4 FMAs) and are rounded once.  Measured at 16 x 256^2 (tools/
//                       thin_train_time.py) the kernel is bound by its FMAs and thin loads, not by the read of the wide tensor.
// The order of every sum is in the header; tests/_thin_train_ref.py restates it.  No atomics anywhere.
#include "ps_common.h"

#include <algorithm>

#include "../../include/pixelsynth_thin_train.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int GW_CT = 32, GW_LANES = GW_CT / 4, GW_GROUPS = THREADS / GW_LANES;      // channels of a workgroup; its lanes per pixel; its pixel groups
static_assert(GW_GROUPS == PS_THIN_TRAIN_GROUPS, "the header states the number of groups");
constexpr int EX_PX = 4, EX_ROWS = 8;                                                              // k_thin_expand: pixels of a row per thread; rows per workgroup

inline bool sizes_ok(int B, int H, int W, int Cw, int T, int k)
{
    return B > 0 && H > 0 && W > 0 && (size_t)B * H * W < ((size_t)1 << 31) && Cw > 0 && Cw % 32 == 0 && Cw <= PS_THIN_TRAIN_MAX_WIDE &&
           T >= 1 && T <= 4 && (k == 1 || k == 3);
}

struct GwPlan {
    size_t npix, part_pix, stride, bytes;      // pixels; pixels of a part; floats of a part's slab (k k T Cw, then the bias's slot of Cw doubles); bytes of the workspace
    int parts;
};

// The split of the pixels: a function of B H W alone (the header's formula).  The bias's slot of a slab holds Cw doubles.
inline GwPlan gw_plan(int B, int H, int W, int Cw, int T, int k)
{
    GwPlan p;
    p.npix = (size_t)B * H * W;
    const size_t steps = (p.npix + GW_GROUPS - 1) / GW_GROUPS;
    p.part_pix = std::max<size_t>(PS_THIN_TRAIN_MIN_PART, GW_GROUPS * ((steps + PS_THIN_TRAIN_MAX_PARTS - 1) / PS_THIN_TRAIN_MAX_PARTS));
    p.parts = (int)((p.npix + p.part_pix - 1) / p.part_pix);
    p.stride = (size_t)k * k * T * Cw + 2 * Cw;
    p.bytes = ps::align_up((size_t)p.parts * p.stride * sizeof(float), 256);
    return p;
}

// a thin pixel's T channels as a float4 (zeros beyond T); T = 4: one 16-byte load
template <int T> __device__ __forceinline__ f32x4 thin_pixel(const float *p)
{
    if (T == 4) return *(const f32x4 *)p;
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < T; ++j) v[j] = p[j];
    return v;
}

__device__ __forceinline__ f32x4 fma4(float s, f32x4 v, f32x4 acc)
{
    const f32x4 ss = {s, s, s, s};
    return __builtin_elementwise_fma(ss, v, acc);
}

// ---- wide from thin ------------------------------------------------------------------------------------------------------------------
template <int T, int K>
__global__ __launch_bounds__(THREADS) void k_thin_expand(const float *__restrict__ g, const float *__restrict__ w, unsigned rows, int H, int W,
                                                        int C4, float *__restrict__ out)
{
    constexpr int TAPS = K * K, R = K / 2, NX = EX_PX + 2 * R;
    __shared__ f32x4 sW[TAPS * T * (PS_THIN_TRAIN_MAX_WIDE / 4)];      // [tap][j][c / 4]
    for (int i = threadIdx.x; i < TAPS * T * C4; i += THREADS) sW[i] = ((const f32x4 *)w)[i];
    __syncthreads();
    // a workgroup: 256 of the (W / 4) C4 items -- (group of four pixels, four channels) -- of EX_ROWS consecutive rows of the batch (the
    // weights are staged once for all of them)
    const unsigned item = blockIdx.y * THREADS + threadIdx.x;
    if (item >= (unsigned)(W / EX_PX) * C4) return;
    const int c4 = (int)(item % (unsigned)C4), x0 = (int)(item / (unsigned)C4) * EX_PX;
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    for (unsigned row = blockIdx.x * EX_ROWS; row < std::min(rows, (blockIdx.x + 1) * EX_ROWS); ++row) {      // frame * H + y
        const int y = (int)(row % (unsigned)H);
        f32x4 acc[EX_PX];
#pragma unroll
        for (int px = 0; px < EX_PX; ++px) acc[px] = zero;
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int yy = y + ky - R;
            if (yy < 0 || yy >= H) continue;
            const float *gr = g + ((size_t)row + ky - R) * (size_t)W * T;           // (yy is inside the frame, so the row exists)
            f32x4 gv[NX];
            bool on[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                const int xx = x0 - R + i;
                on[i] = xx >= 0 && xx < W;
                gv[i] = on[i] ? thin_pixel<T>(gr + (size_t)xx * T) : zero;
            }
#pragma unroll
            for (int kx = 0; kx < K; ++kx)
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    const f32x4 wv = sW[((ky * K + kx) * T + j) * C4 + c4];
#pragma unroll
                    for (int px = 0; px < EX_PX; ++px)
                        if (on[px + kx]) acc[px] = fma4(gv[px + kx][j], wv, acc[px]);
                }
        }
        float *dst = out + (((size_t)row * W + x0) * (size_t)C4 + c4) * 4;
#pragma unroll
        for (int px = 0; px < EX_PX; ++px) *(f32x4 *)(dst + (size_t)px * C4 * 4) = acc[px];
    }
}

// ---- the weight and bias gradient ------------------------------------------------------------------------------------------------------
struct GwArgs {
    const float *thin, *wide;
    int H, W, Cw, sign, wide_is_g, with_bias;
    size_t npix, part_pix, stride;
    float *slab;
};

template <int T, int K>
__global__ __launch_bounds__(THREADS) void k_thin_grad_weight(GwArgs a)
{
    constexpr int TAPS = K * K, R = K / 2, NA = TAPS * T, CHUNK = 4;
    __shared__ f32x4 sRed[CHUNK][THREADS];      // (16 KB; the bias's 256 x 4 doubles take the first half of it afterwards)
    const int tid = threadIdx.x, lane = tid & (GW_LANES - 1), grp = tid / GW_LANES;
    const int H = a.H, W = a.W, Cw = a.Cw, c = (int)blockIdx.x * GW_CT + 4 * lane;
    const size_t lo = (size_t)blockIdx.y * a.part_pix, hi = std::min(a.npix, lo + a.part_pix);
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 acc[NA];
    double bs[4] = {0.0, 0.0, 0.0, 0.0};        // the bias's sums: fp64 all the way, rounded once by k_thin_sum_parts
#pragma unroll
    for (int i = 0; i < NA; ++i) acc[i] = zero;
    // (x, y) of the thread's pixel advance with it: no division in the loop.  A pixel whose taps all lie inside the frame -- all but the
    // frame's border -- takes them without a test; the order of the terms is the same on both paths.
    size_t p = lo + grp;
    int x = (int)(p % W), y = (int)((p / W) % H);
    const int xstep = GW_GROUPS % W, ystep = GW_GROUPS / W;
    const ptrdiff_t rowoff = (ptrdiff_t)a.sign * W * T, coloff = (ptrdiff_t)a.sign * T;
    for (; p < hi; p += GW_GROUPS) {
        const f32x4 wv = *(const f32x4 *)(a.wide + p * (size_t)Cw + c);
        const float *tp = a.thin + p * (size_t)T;
        if (y >= R && y + R < H && x >= R && x + R < W) {
#pragma unroll
            for (int ky = 0; ky < K; ++ky)
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const f32x4 tv = thin_pixel<T>(tp + (ky - R) * rowoff + (kx - R) * coloff);
#pragma unroll
                    for (int j = 0; j < T; ++j) acc[(ky * K + kx) * T + j] = fma4(tv[j], wv, acc[(ky * K + kx) * T + j]);
                }
        } else {
#pragma unroll
            for (int ky = 0; ky < K; ++ky)
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const int dy = a.sign * (ky - R), dx = a.sign * (kx - R);
                    if (y + dy < 0 || y + dy >= H || x + dx < 0 || x + dx >= W) continue;
                    const f32x4 tv = thin_pixel<T>(tp + (ky - R) * rowoff + (kx - R) * coloff);
#pragma unroll
                    for (int j = 0; j < T; ++j) acc[(ky * K + kx) * T + j] = fma4(tv[j], wv, acc[(ky * K + kx) * T + j]);
                }
        }
        if (a.with_bias) {
            const f32x4 bv = a.wide_is_g ? wv : thin_pixel<T>(tp);
#pragma unroll
            for (int r = 0; r < 4; ++r) bs[r] += (double)bv[r];
        }
        x += xstep;
        y += ystep;
        if (x >= W) {
            x -= W;
            ++y;
        }
        if (y >= H) y %= H;
    }

    // the groups in ascending order, CHUNK accumulators at a time: thread (i, lane) of the first CHUNK * 8 adds accumulator a0 + i
    float *dst = a.slab + (size_t)blockIdx.y * a.stride;
#pragma unroll
    for (int a0 = 0; a0 < NA; a0 += CHUNK) {
#pragma unroll
        for (int i = 0; i < CHUNK; ++i)
            if (a0 + i < NA) sRed[i][tid] = acc[a0 + i];
        __syncthreads();
        const int i = tid / GW_LANES, ai = a0 + i;
        if (tid < CHUNK * GW_LANES && ai < NA) {
            f32x4 v = sRed[i][lane];
            for (int q = 1; q < GW_GROUPS; ++q) v = v + sRed[i][q * GW_LANES + lane];
            *(f32x4 *)(dst + (size_t)ai * Cw + c) = v;
        }
        __syncthreads();
    }
    if (!a.with_bias) return;      // (uniform)
    // the bias's slot follows the accumulators': Cw doubles.  The thin side's sums are the same in every lane and channel tile: lane 0 of tile 0 stores them
    double *sB = (double *)&sRed[0][0], *dstb = (double *)(dst + (size_t)NA * Cw);
#pragma unroll
    for (int r = 0; r < 4; ++r) sB[tid * 4 + r] = bs[r];
    __syncthreads();
    if (tid < GW_LANES && (a.wide_is_g || (blockIdx.x == 0 && lane == 0))) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double v = sB[lane * 4 + r];
            for (int q = 1; q < GW_GROUPS; ++q) v += sB[(q * GW_LANES + lane) * 4 + r];
            dstb[(a.wide_is_g ? c : 0) + r] = v;
        }
    }
}

// out_w[e] = slab[0][e] + slab[1][e] + ... in ascending part for the nw4 float4s of the weight's gradient; the nb sums of the bias's likewise
// in fp64 (a part's Cw doubles lie `bias_at` floats into its slab), rounded to fp32 once
__global__ __launch_bounds__(THREADS) void k_thin_sum_parts(const float *__restrict__ slab, int parts, size_t stride, int nw4, int nb, size_t bias_at,
                                                           f32x4 *__restrict__ out_w, float *__restrict__ out_b)
{
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e < nw4) {
        f32x4 v = ((const f32x4 *)slab)[e];
#pragma unroll 32      // (the loads of 32 parts in flight; the adds stay in ascending order)
        for (int p = 1; p < parts; ++p) v = v + ((const f32x4 *)(slab + (size_t)p * stride))[e];
        out_w[e] = v;
    } else if (e - nw4 < nb) {
        double v = ((const double *)(slab + bias_at))[e - nw4];
#pragma unroll 32
        for (int p = 1; p < parts; ++p) v += ((const double *)(slab + (size_t)p * stride + bias_at))[e - nw4];
        out_b[e - nw4] = (float)v;
    }
}

// ---- the bias of a forward pass --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_thin_add_bias4(f32x4 *__restrict__ y, const f32x4 *__restrict__ bias, int C4, size_t total4)
{
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < total4; i += (size_t)gridDim.x * THREADS) y[i] = y[i] + bias[i % C4];
}

__global__ __launch_bounds__(THREADS) void k_thin_add_bias1(float *__restrict__ y, const float *__restrict__ bias, int C, size_t total)
{
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * THREADS) y[i] = y[i] + bias[i % C];
}

unsigned grid_for(size_t total) { return (unsigned)std::min<size_t>((total + THREADS - 1) / THREADS, 256 * 32); }

using ps::aligned16;

inline bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }

template <int T, int K> int launch_expand(const float *g, const float *w, int B, int H, int W, int Cw, float *out, hipStream_t st)
{
    const unsigned items = (unsigned)(W / EX_PX) * (Cw / 4);            // of a row; at most 65535 * 256 (checked by the caller)
    hipLaunchKernelGGL((k_thin_expand<T, K>), dim3(((unsigned)B * H + EX_ROWS - 1) / EX_ROWS, (items + THREADS - 1) / THREADS), dim3(THREADS),
                       0, st, g, w, (unsigned)B * H, H, W, Cw / 4, out);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

template <int T, int K> int launch_grad_weight(const GwArgs &a, int parts, hipStream_t st)
{
    hipLaunchKernelGGL((k_thin_grad_weight<T, K>), dim3(a.Cw / GW_CT, parts), dim3(THREADS), 0, st, a);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

// f<T, K>(args...) for the runtime T in 1 .. 4 and k in {1, 3}
#define PS_THIN_DISPATCH(f, T, k, ...)                                     \
    ((k) == 1 ? ((T) == 1   ? f<1, 1>(__VA_ARGS__)                         \
                 : (T) == 2 ? f<2, 1>(__VA_ARGS__)                         \
                 : (T) == 3 ? f<3, 1>(__VA_ARGS__)                         \
                            : f<4, 1>(__VA_ARGS__))                        \
              : ((T) == 1   ? f<1, 3>(__VA_ARGS__)                         \
                 : (T) == 2 ? f<2, 3>(__VA_ARGS__)                         \
                 : (T) == 3 ? f<3, 3>(__VA_ARGS__)                         \
                            : f<4, 3>(__VA_ARGS__)))

}  // namespace

extern "C" {

const char *ps_thin_train_last_error(void) { return ps::last_error_ref().c_str(); }

int ps_thin_train_parts(int B, int H, int W, int Cw, int T, int k) { return sizes_ok(B, H, W, Cw, T, k) ? gw_plan(B, H, W, Cw, T, k).parts : 0; }

size_t ps_thin_train_workspace_bytes(int B, int H, int W, int Cw, int T, int k)
{
    return sizes_ok(B, H, W, Cw, T, k) ? gw_plan(B, H, W, Cw, T, k).bytes : 0;
}

int ps_thin_expand_f32(const float *g, const float *w, int B, int H, int W, int T, int Cw, int k, float *out, void *stream)
{
    PS_REQUIRE(g && w && out, "thin_expand: null pointer");
    PS_REQUIRE(sizes_ok(B, H, W, Cw, T, k) && W % EX_PX == 0,
               "thin_expand: W a multiple of 4, Cw a multiple of 32 up to %d, 1 <= T <= 4, k 1 or 3 and B H W < 2^31 required (B = %d, H = %d, W = %d, "
               "T = %d, Cw = %d, k = %d)", PS_THIN_TRAIN_MAX_WIDE, B, H, W, T, Cw, k);
    PS_REQUIRE((size_t)(W / EX_PX) * (Cw / 4) <= (size_t)65535 * THREADS, "thin_expand: rows of %d pixels are too long", W);
    PS_REQUIRE(aligned16(w) && aligned16(out) && (T == 4 ? aligned16(g) : aligned4(g)),
               "thin_expand: w, out and a four-channel g must be aligned to 16 bytes, any other g to 4");
    return PS_THIN_DISPATCH(launch_expand, T, k, g, w, B, H, W, Cw, out, (hipStream_t)stream);
}

int ps_thin_grad_weight_f32(const float *thin, const float *wide, int B, int H, int W, int Cw, int T, int k, int wide_is_g,
                            float *grad_weight, float *grad_bias, void *workspace, size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(thin && wide && grad_weight, "thin_grad_weight: null pointer");
    PS_REQUIRE(sizes_ok(B, H, W, Cw, T, k),
               "thin_grad_weight: Cw a multiple of 32 up to %d, 1 <= T <= 4, k 1 or 3 and B H W < 2^31 required (B = %d, H = %d, W = %d, Cw = %d, "
               "T = %d, k = %d)", PS_THIN_TRAIN_MAX_WIDE, B, H, W, Cw, T, k);
    PS_REQUIRE(wide_is_g == 0 || wide_is_g == 1, "thin_grad_weight: wide_is_g is 0 or 1 (%d)", wide_is_g);
    PS_REQUIRE(aligned16(wide) && aligned16(grad_weight) && aligned4(grad_bias) && (T == 4 ? aligned16(thin) : aligned4(thin)),
               "thin_grad_weight: wide, grad_weight and a four-channel thin must be aligned to 16 bytes, any other thin and grad_bias to 4");
    const GwPlan p = gw_plan(B, H, W, Cw, T, k);
    PS_REQUIRE(workspace, "thin_grad_weight: null pointer (workspace)");
    PS_REQUIRE(workspace_bytes >= p.bytes, "thin_grad_weight: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    PS_REQUIRE(aligned16(workspace), "thin_grad_weight: the workspace must be aligned to 16 bytes");
    hipStream_t st = (hipStream_t)stream;
    GwArgs a{thin, wide, H, W, Cw, wide_is_g ? 1 : -1, wide_is_g, grad_bias != nullptr, p.npix, p.part_pix, p.stride, (float *)workspace};
    const int rc = PS_THIN_DISPATCH(launch_grad_weight, T, k, a, p.parts, st);
    if (rc != PS_OK) return rc;
    const int nw4 = k * k * T * Cw / 4, nb = grad_bias ? (wide_is_g ? Cw : T) : 0;
    hipLaunchKernelGGL(k_thin_sum_parts, dim3((nw4 + nb + THREADS - 1) / THREADS), dim3(THREADS), 0, st, (const float *)workspace, p.parts,
                       p.stride, nw4, nb, (size_t)nw4 * 4, (f32x4 *)grad_weight, grad_bias);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_thin_add_bias_f32(float *y, const float *bias, size_t npix, int C, void *stream)
{
    PS_REQUIRE(y && bias, "thin_add_bias: null pointer");
    PS_REQUIRE(npix > 0 && C > 0, "thin_add_bias: npix and C >= 1 required (npix = %zu, C = %d)", npix, C);
    if (C % 4 == 0 && aligned16(y) && aligned16(bias))
        hipLaunchKernelGGL(k_thin_add_bias4, dim3(grid_for(npix * (C / 4))), dim3(THREADS), 0, (hipStream_t)stream, (f32x4 *)y,
                           (const f32x4 *)bias, C / 4, npix * (C / 4));
    else
        hipLaunchKernelGGL(k_thin_add_bias1, dim3(grid_for(npix * C)), dim3(THREADS), 0, (hipStream_t)stream, y, bias, C, npix * C);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
