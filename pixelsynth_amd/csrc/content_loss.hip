// content_loss.hip -- what lies between the convolutions of the VGG19 content loss (the reference's models/losses/synthesis.py:85-104:
// PerceptualLoss, the L1 of five VGG19 feature maps), forward and backward, for gfx950 (MI355X).  Behind the C ABI of
// include/pixelsynth_content.h (libpixelsynth_content.so, beside libpixelsynth_hip.so whose set of exports it leaves as it is).  The
// thirteen convolutions and their grad_input twins are conv_thin.hip's and conv_f16x3.hip's kernels, the gradient's scale conv_bwd.hip's.
//
//   k_input    one thread per pixel of an image: pred / gt (P, 3, H, W) through element strides -> (2P, H, W, 4), channel 3 zero.
//   k_bias     y += bias[c] in place (conv1_1's bias, added once).
//   k_tap      one workgroup per tile of 256 prediction pixels: |relu(a) - relu(b)| in fp64, one chain per thread, a fixed tree.
//   k_finish   one workgroup: per level the tiles staged through LDS 256 at a time and added by ONE thread in ascending order.
//   k_pool     the 2 x 2 max-pool of a pre-ReLU map, a NaN kept.
//   k_join     the backward pass between two grad_input convolutions: unscale, route through the pool, add the L1 term's seed, mask
//              by the ReLU -- one read of y (and y_gt), one of up, one write.  With a pool between, a thread owns a window.
// Every kernel moves 16 bytes per lane and access; all but k_tap / k_finish are grid-stride loops over float4 elements.  No atomics.
#include "ps_image.h"
#include "../../include/pixelsynth_content.h"

#include <algorithm>

namespace {

using ps::aligned16;
using ps::f32x4;
using ps::Img;
using ps::max4_keep_nan;

constexpr int THREADS = PS_CONTENT_THREADS, TILE = PS_CONTENT_TILE, LEVELS = PS_CONTENT_LEVELS;

__global__ __launch_bounds__(256) void k_input(Img a, Img b, int P, int H, int W, f32x4 *__restrict__ out)
{
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int img = blockIdx.y;
    if (pix >= (size_t)H * W) return;
    const int h = (int)(pix / W), w = (int)(pix - (size_t)h * W);
    const Img &im = img < P ? a : b;
    const float *p = (const float *)im.p + (long long)(img < P ? img : img - P) * im.sB + (long long)h * im.sH + (long long)w * im.sW;
    const f32x4 o = {p[0], p[im.sC], p[2 * im.sC], 0.0f};
    out[(size_t)img * H * W + pix] = o;
}

__global__ __launch_bounds__(256) void k_bias(f32x4 *__restrict__ y, const f32x4 *__restrict__ bias, int C4, size_t total4)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total4; e += (size_t)gridDim.x * 256) y[e] = y[e] + bias[e % C4];
}

__global__ __launch_bounds__(THREADS) void k_tap(const f32x4 *__restrict__ y, size_t npix, int C4, double *__restrict__ sums)
{
    __shared__ double red[THREADS];
    const int tid = threadIdx.x;
    const size_t tile = blockIdx.x, n0 = tile * TILE, n1 = std::min(npix, n0 + TILE);
    const f32x4 *a = y + n0 * C4, *b = y + (npix + n0) * C4;
    const size_t count = (n1 - n0) * C4;
    double s = 0.0;
#pragma unroll 4
    for (size_t e = tid; e < count; e += THREADS) {
        const f32x4 ra = ps::relu_keep_nan(a[e]), rb = ps::relu_keep_nan(b[e]);
#pragma unroll
        for (int j = 0; j < 4; ++j) s += fabs((double)ra[j] - (double)rb[j]);
    }
    red[tid] = s;
    PS_BLOCK_TREE_SUM(red, tid, 1, THREADS);
    if (tid == 0) sums[tile] = red[0];
}

struct Finish {
    long long tiles[LEVELS], counts[LEVELS];
};

__global__ __launch_bounds__(THREADS) void k_finish(const double *__restrict__ sums, Finish f, float *__restrict__ levels,
                                                    float *__restrict__ total)
{
    __shared__ double stage[THREADS];
    const int tid = threadIdx.x;
    const double *blk = sums;
    const double weights[LEVELS] = {1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0};
    double tot = 0.0;
    for (int l = 0; l < LEVELS; ++l) {
        const double w = weights[l];
        const long long tiles = f.tiles[l];
        double s = 0.0;                              // (thread 0's: the level's one chain)
        for (long long t0 = 0; t0 < tiles; t0 += THREADS) {
            if (t0 + tid < tiles) stage[tid] = blk[t0 + tid];
            __syncthreads();
            if (tid == 0) {
                const int n = (int)std::min<long long>(THREADS, tiles - t0);
                for (int k = 0; k < n; ++k) s += stage[k];
            }
            __syncthreads();
        }
        if (tid == 0) {
            const double L = tiles > 0 ? s / (double)f.counts[l] : 0.0;
            levels[l] = (float)L;
            if (tiles > 0) tot += w * L;
        }
        blk += tiles;
    }
    if (tid == 0) total[0] = (float)tot;
}

// float4 index of pixel (y, x) of image f in a (., H, W, C4) map
__device__ __forceinline__ size_t at(size_t f, int y, int x, int H, int W, int C4) { return ((f * H + y) * W + x) * (size_t)C4; }

__global__ __launch_bounds__(256) void k_pool(const f32x4 *__restrict__ y, int H, int W, int C4, size_t total4, f32x4 *__restrict__ out)
{
    const int Ho = H / 2, Wo = W / 2;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total4; e += (size_t)gridDim.x * 256) {
        const int c4 = (int)(e % C4);
        size_t p = e / C4;
        const int qx = (int)(p % Wo);
        p /= Wo;
        const int qy = (int)(p % Ho);
        const size_t f = p / Ho;
        const f32x4 *w = y + at(f, 2 * qy, 2 * qx, H, W, C4) + c4;
        out[e] = max4_keep_nan(w[0], w[C4], w[(size_t)W * C4], w[(size_t)W * C4 + C4]);
    }
}

struct Join {
    const f32x4 *y, *y_gt, *up;
    const float *scale2, *g;
    float weight, count;
    int H, W, C4;
    size_t total4;          // the float4 elements a thread loop runs over: of y, or of up where a pool lies between
    f32x4 *G;
};

// c * sign(relu(a) - relu(b)), per channel: torch.sign's (0 < d) - (d < 0), 0 for a NaN
__device__ __forceinline__ f32x4 seed(f32x4 a, f32x4 b, float c)
{
    const f32x4 d = ps::relu_keep_nan(a) - ps::relu_keep_nan(b);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = c * ((float)(0.0f < d[j]) - (float)(d[j] < 0.0f));
    return o;
}

// threshold_backward: 0 where y <= 0, the gradient elsewhere (a NaN of y included)
__device__ __forceinline__ f32x4 masked(f32x4 y, f32x4 v)
{
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = y[j] <= 0.0f ? 0.0f : v[j];
    return o;
}

template <bool UP, bool SEED> __global__ __launch_bounds__(256) void k_join(Join a)
{
    const float inv_s = UP ? a.scale2[1] : 0.0f;
    const float c = SEED ? (a.g[0] * a.weight) / a.count : 0.0f;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < a.total4; e += (size_t)gridDim.x * 256) {
        const f32x4 yv = a.y[e];
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (UP) v = a.up[e] * inv_s;
        if (SEED) {
            const f32x4 s = seed(yv, a.y_gt[e], c);
            v = UP ? v + s : s;
        }
        a.G[e] = masked(yv, v);
    }
}

// a pool between: a thread owns the window of one element of up
template <bool SEED> __global__ __launch_bounds__(256) void k_join_pooled(Join a)
{
    const float inv_s = a.scale2[1];
    const float c = SEED ? (a.g[0] * a.weight) / a.count : 0.0f;
    const int H = a.H, W = a.W, C4 = a.C4, Ho = H / 2, Wo = W / 2;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < a.total4; e += (size_t)gridDim.x * 256) {
        const int c4 = (int)(e % C4);
        size_t p = e / C4;
        const int qx = (int)(p % Wo);
        p /= Wo;
        const int qy = (int)(p % Ho);
        const size_t f = p / Ho;
        const size_t base = at(f, 2 * qy, 2 * qx, H, W, C4) + c4;
        const size_t off[4] = {base, base + C4, base + (size_t)W * C4, base + (size_t)W * C4 + C4};
        f32x4 yv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) yv[k] = a.y[off[k]];
        const f32x4 u = a.up[e] * inv_s;
        int best[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float val = yv[0][j];
            best[j] = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                const float t = yv[k][j];
                if (t > val || t != t) {
                    val = t;
                    best[j] = k;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = best[j] == k ? u[j] : 0.0f;
            if (SEED) v = v + seed(yv[k], a.y_gt[off[k]], c);
            a.G[off[k]] = masked(yv[k], v);
        }
    }
}

unsigned grid_for(size_t total4) { return (unsigned)std::min<size_t>((total4 + 255) / 256, 256 * 32); }


// what every map-shaped call asks of its sizes
inline bool map_ok(long long N, int H, int W, int C)
{
    return N >= 1 && H >= 1 && W >= 1 && C >= 64 && C % 64 == 0 && (size_t)N * H * W <= ((size_t)1 << 40) / C;
}

}  // namespace

extern "C" {

const char *ps_content_last_error(void) { return ps::last_error_ref().c_str(); }

size_t ps_content_tiles(size_t npix) { return (npix + TILE - 1) / TILE; }

int ps_content_input(const float *pred, const int64_t *strides_pred, const float *gt, const int64_t *strides_gt, int P, int H, int W,
                     float *out, void *stream)
{
    PS_REQUIRE(pred && gt && strides_pred && strides_gt && out, "content_input: null pointer");
    PS_REQUIRE(P >= 1 && P <= 32767, "content_input: 1 <= P <= 32767 required (P = %d)", P);
    for (int i = 0; i < 4; ++i) PS_REQUIRE(strides_pred[i] >= 0 && strides_gt[i] >= 0, "content_input: negative stride");
    PS_REQUIRE(H >= 1 && W >= 1 && (size_t)H * W < ((size_t)1 << 31), "content_input: H = %d, W = %d", H, W);
    PS_REQUIRE(aligned16(out), "content_input: out must be aligned to 16 bytes");
    const Img a(pred, strides_pred), b(gt, strides_gt);
    const dim3 grid((unsigned)(((size_t)H * W + 255) / 256), 2 * P);
    hipLaunchKernelGGL(k_input, grid, dim3(256), 0, (hipStream_t)stream, a, b, P, H, W, (f32x4 *)out);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_content_bias(float *y, const float *bias, size_t npix, int C, void *stream)
{
    PS_REQUIRE(y && bias, "content_bias: null pointer");
    PS_REQUIRE(map_ok((long long)npix, 1, 1, C), "content_bias: npix >= 1 and C a multiple of 64 required (npix = %zu, C = %d)", npix, C);
    PS_REQUIRE(aligned16(y) && aligned16(bias), "content_bias: buffers must be aligned to 16 bytes");
    const size_t total4 = npix * (C / 4);
    hipLaunchKernelGGL(k_bias, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, (f32x4 *)y, (const f32x4 *)bias, C / 4, total4);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_content_tap(const float *y, int P, int Hl, int Wl, int C, double *sums, void *stream)
{
    PS_REQUIRE(y && sums, "content_tap: null pointer");
    PS_REQUIRE(map_ok(2LL * P, Hl, Wl, C), "content_tap: P, Hl, Wl >= 1 and C a multiple of 64 required (P = %d, Hl = %d, Wl = %d, C = %d)",
               P, Hl, Wl, C);
    PS_REQUIRE(aligned16(y) && ((uintptr_t)sums & 7) == 0, "content_tap: y must be aligned to 16 bytes, sums to 8");
    const size_t npix = (size_t)P * Hl * Wl, tiles = ps_content_tiles(npix);
    PS_REQUIRE(tiles < ((size_t)1 << 31), "content_tap: too many tiles");
    hipLaunchKernelGGL(k_tap, dim3((unsigned)tiles), dim3(THREADS), 0, (hipStream_t)stream, (const f32x4 *)y, npix, C / 4, sums);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_content_finish(const double *sums, const int64_t *tiles, const int64_t *counts, float *levels, float *total, void *stream)
{
    PS_REQUIRE(sums && tiles && counts && levels && total, "content_finish: null pointer");
    Finish f;
    for (int l = 0; l < LEVELS; ++l) {
        PS_REQUIRE(tiles[l] >= 0 && (tiles[l] == 0 || counts[l] >= 1), "content_finish: level %d: tiles = %lld, count = %lld", l,
                   (long long)tiles[l], (long long)counts[l]);
        f.tiles[l] = tiles[l];
        f.counts[l] = counts[l];
    }
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, sums, f, levels, total);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_content_pool(const float *y, int N, int Hl, int Wl, int C, float *pooled, void *stream)
{
    PS_REQUIRE(y && pooled, "content_pool: null pointer");
    PS_REQUIRE(map_ok(N, Hl, Wl, C) && Hl % 2 == 0 && Wl % 2 == 0,
               "content_pool: N >= 1, even Hl and Wl and C a multiple of 64 required (N = %d, Hl = %d, Wl = %d, C = %d)", N, Hl, Wl, C);
    PS_REQUIRE(aligned16(y) && aligned16(pooled), "content_pool: buffers must be aligned to 16 bytes");
    const size_t total4 = (size_t)N * (Hl / 2) * (Wl / 2) * (C / 4);
    hipLaunchKernelGGL(k_pool, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, (const f32x4 *)y, Hl, Wl, C / 4, total4,
                       (f32x4 *)pooled);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_content_join(const float *y, const float *y_gt, const float *up, const float *scale2, const float *g, float weight, int P, int Hl,
                    int Wl, int C, int pooled, float *G, void *stream)
{
    PS_REQUIRE(y && G, "content_join: null pointer");
    PS_REQUIRE(up || y_gt, "content_join: neither up nor y_gt");
    PS_REQUIRE(!up || scale2, "content_join: up without scale2");
    PS_REQUIRE(!y_gt || g, "content_join: y_gt without g");
    PS_REQUIRE(!pooled || up, "content_join: a pool without up");
    PS_REQUIRE(map_ok(P, Hl, Wl, C) && (!pooled || (Hl % 2 == 0 && Wl % 2 == 0)),
               "content_join: P >= 1, C a multiple of 64 and, with a pool, even Hl and Wl required (P = %d, Hl = %d, Wl = %d, C = %d)", P, Hl,
               Wl, C);
    PS_REQUIRE(aligned16(y) && aligned16(y_gt) && aligned16(up) && aligned16(G), "content_join: buffers must be aligned to 16 bytes");
    PS_REQUIRE(G != y && G != y_gt && G != up, "content_join: G must not be an input");
    const size_t npix = (size_t)P * Hl * Wl;
    Join a{(const f32x4 *)y, (const f32x4 *)y_gt, (const f32x4 *)up, scale2, g, weight, (float)((double)npix * C), Hl, Wl, C / 4,
           (pooled ? npix / 4 : npix) * (C / 4), (f32x4 *)G};
    const dim3 grid(grid_for(a.total4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (pooled) {
        if (y_gt)
            hipLaunchKernelGGL(k_join_pooled<true>, grid, block, 0, st, a);
        else
            hipLaunchKernelGGL(k_join_pooled<false>, grid, block, 0, st, a);
    } else if (up && y_gt) {
        hipLaunchKernelGGL((k_join<true, true>), grid, block, 0, st, a);
    } else if (up) {
        hipLaunchKernelGGL((k_join<true, false>), grid, block, 0, st, a);
    } else {
        hipLaunchKernelGGL((k_join<false, true>), grid, block, 0, st, a);
    }
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
