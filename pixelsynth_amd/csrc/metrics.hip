// metrics.hip -- per-image PSNR and SSIM of a batch of image pairs, with an optional per-pixel mask, for gfx950 (MI355X): the reference's
// evaluation metrics (evaluation/metrics.py:6-23, models/losses/ssim.py:12-124, calc_errors_quality.py:28-77) in two launches.
//
//   k_metrics_tiles   one workgroup per (tile of 32 x 32 output pixels, image), all channels of the tile.  Per channel: the (32 + 10)^2
//                     halo of both images is staged in LDS as fp32 (zero outside the image: the reference's padding of 5); a horizontal
//                     11-tap pass writes the five moment maps (x, y, x^2, y^2, x y) of the 42 x 32 rows to LDS in fp64; a vertical pass
//                     in registers (four consecutive output rows per thread, 14 loads per map) finishes them.  sigma = E[x^2] - mu^2 is
//                     then formed in fp64, so flat regions do not cancel as the fp32 formula does.  The SSIM map and the squared
//                     differences accumulate over the channels in registers; the 8 per-tile sums below are reduced over the workgroup in
//                     a fixed tree order and written to the workspace.  No atomics.
//   k_metrics_finish  one thread per image: the tile sums in tile order, fp64, then the six numbers.
//
// The window is the product of the reference's fp32 1-D taps (gaussian(11, 1.5) normalised in fp32), formed exactly in fp64.  The reference
// rounds each 2-D tap g_i g_j to fp32 (create_window); the two windows differ by at most half an fp32 ulp per tap.
//
// Per-tile sums (fp64), m = mask, n = 1 - m (fp32, as the caller of the reference forms it):
//   0: sum_c,p d^2     1: sum_p m sum_c d^2     2: sum_p n sum_c d^2     3: sum_p m     4: sum_p n
//   5: sum_c,p ssim    6: sum_p m mean_c ssim   7: sum_p n mean_c ssim                 (d = x - y in fp32, squared in fp32)
#include "ps_image.h"

#include <cmath>

namespace {

using ps::Img;
using ps::to_unit;

constexpr int MT = 32;                   // output tile edge
constexpr int MR = 5;                    // window radius
constexpr int MH = MT + 2 * MR;          // staged halo edge (42)
constexpr int M_THREADS = 256;           // 32 columns x 8 row groups of 4 rows
constexpr int M_SUMS = 8;

// gaussian(11, 1.5) / its fp32 sum, as models/losses/ssim.py:12-19 builds it in fp32 (tests/test_metrics_cpu.py re-derives them)
__constant__ float c_gauss[11] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.106560p-2f,
                                  0x1.b43c3ep-3f,  0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};

template <typename T>
__global__ __launch_bounds__(M_THREADS) void k_metrics_tiles(Img a, Img b, const float *mask, int C, int H, int W, int tiles_x,
                                                             double *ws)
{
    __shared__ float sa[MH * MH], sb[MH * MH];
    __shared__ double hm[5 * MH * MT];                   // [map][row][col]; reused for the reduction
    const int tid = threadIdx.x, lx = tid & (MT - 1), ly = tid >> 5;
    const int tile = blockIdx.x, img = blockIdx.y;
    const int y0 = (tile / tiles_x) * MT, x0 = (tile % tiles_x) * MT;
    const T *pa = (const T *)a.p + (long long)img * a.sB, *pb = (const T *)b.p + (long long)img * b.sB;
    double g[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) g[k] = (double)c_gauss[k];
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;

    double ssim_c[4] = {0.0, 0.0, 0.0, 0.0}, d2_c[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < C; ++c) {
        for (int e = tid; e < MH * MH; e += M_THREADS) {
            const int r = e / MH, q = e - r * MH, gy = y0 - MR + r, gx = x0 - MR + q;
            float va = 0.0f, vb = 0.0f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                va = to_unit<T>(pa[c * a.sC + gy * a.sH + gx * a.sW]);
                vb = to_unit<T>(pb[c * b.sC + gy * b.sH + gx * b.sW]);
            }
            sa[e] = va;
            sb[e] = vb;
        }
        __syncthreads();
        for (int e = tid; e < MH * MT; e += M_THREADS) {   // horizontal pass: row r of the halo, output column q
            const int r = e >> 5, q = e & (MT - 1);
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const double x = (double)sa[r * MH + q + k], y = (double)sb[r * MH + q + k];
                s0 = fma(g[k], x, s0);
                s1 = fma(g[k], y, s1);
                s2 = fma(g[k], x * x, s2);               // x * x, y * y, x * y of fp32 values are exact in fp64
                s3 = fma(g[k], y * y, s3);
                s4 = fma(g[k], x * y, s4);
            }
            hm[0 * MH * MT + e] = s0;
            hm[1 * MH * MT + e] = s1;
            hm[2 * MH * MT + e] = s2;
            hm[3 * MH * MT + e] = s3;
            hm[4 * MH * MT + e] = s4;
        }
        __syncthreads();
        double o[5][4];
#pragma unroll
        for (int m = 0; m < 5; ++m) {                    // vertical pass: output rows 4 ly .. 4 ly + 3 of column lx
            double v[14];
#pragma unroll
            for (int j = 0; j < 14; ++j) v[j] = hm[m * MH * MT + (4 * ly + j) * MT + lx];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 11; ++k) s = fma(g[k], v[p + k], s);
                o[m][p] = s;
            }
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const double mu1 = o[0][p], mu2 = o[1][p], mu12 = mu1 * mu2;
            const double s11 = o[2][p] - mu1 * mu1, s22 = o[3][p] - mu2 * mu2, s12 = o[4][p] - mu12;
            ssim_c[p] += ((2.0 * mu12 + C1) * (2.0 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2));
            const int ci = (4 * ly + p + MR) * MH + lx + MR;
            const float d = sa[ci] - sb[ci], d2 = d * d;
            d2_c[p] += (double)d2;
        }
        __syncthreads();                                 // before the next channel's staging overwrites sa / sb / hm
    }

    double s[M_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int gy = y0 + 4 * ly + p, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        const float mf = mask ? mask[((long long)img * H + gy) * W + gx] : 0.0f, nf = 1.0f - mf;
        const double m = mf, n = nf, mean_c = ssim_c[p] / (double)C;
        s[0] += d2_c[p];
        s[1] += m * d2_c[p];
        s[2] += n * d2_c[p];
        s[3] += m;
        s[4] += n;
        s[5] += ssim_c[p];
        s[6] += m * mean_c;
        s[7] += n * mean_c;
    }
    double *red = hm;                                    // [sum][thread]
#pragma unroll
    for (int k = 0; k < M_SUMS; ++k) red[k * M_THREADS + tid] = s[k];
    PS_BLOCK_TREE_SUM(red, tid, M_SUMS, M_THREADS);
    if (tid < M_SUMS) ws[((long long)img * gridDim.x + tile) * M_SUMS + tid] = red[tid * M_THREADS];
}

__global__ __launch_bounds__(64) void k_metrics_finish(const double *ws, int B, int tiles, int C, int H, int W, int has_mask, float *out)
{
    const int img = blockIdx.x * 64 + threadIdx.x;
    if (img >= B) return;
    double s[M_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = 0; t < tiles; ++t)
#pragma unroll
        for (int k = 0; k < M_SUMS; ++k) s[k] += ws[((long long)img * tiles + t) * M_SUMS + k];
    const double n = (double)C * H * W;
    float *o = out + (long long)img * 6;
    o[0] = (float)(10.0 * log10(1.0 / (s[0] / n)));
    o[3] = (float)(s[5] / n);
    if (has_mask) {
        // the 3 is the reference's literal (evaluation/metrics.py:17), whatever C is
        const double wv = fmax(s[3], 1.0), wi = fmax(s[4], 1.0);
        o[1] = (float)(10.0 * log10(1.0 / (s[1] / (3.0 * wv))));
        o[2] = (float)(10.0 * log10(1.0 / (s[2] / (3.0 * wi))));
        o[4] = (float)(s[6] / wv);
        o[5] = (float)(s[7] / wi);
    } else {
        o[1] = o[2] = o[4] = o[5] = __builtin_nanf("");
    }
}

int tiles_of(int H, int W) { return ((H + MT - 1) / MT) * ((W + MT - 1) / MT); }

}  // namespace

extern "C" {

size_t ps_image_metrics_workspace_bytes(int B, int C, int H, int W)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * tiles_of(H, W) * M_SUMS * sizeof(double);
}

int ps_image_metrics(const void *img1, const int64_t *strides1, const void *img2, const int64_t *strides2, int dtype, const float *mask,
                     int B, int C, int H, int W, float *out, void *workspace, size_t workspace_bytes, void *stream)
{
    PS_REQUIRE_IMAGES("image_metrics", img1 && img2 && strides1 && strides2 && out, dtype, B, strides1, strides2);
    PS_REQUIRE(C == 1 || C == 3, "image_metrics: C must be 1 or 3 (got %d)", C);
    PS_REQUIRE(H >= 1 && W >= 1, "image_metrics: H, W >= 1 required (H = %d, W = %d)", H, W);
    const size_t need = ps_image_metrics_workspace_bytes(B, C, H, W);
    PS_REQUIRE(workspace && workspace_bytes >= need, "image_metrics: workspace of %zu bytes required (got %zu)", need, workspace_bytes);
    const Img a(img1, strides1), b(img2, strides2);
    const int tiles_x = (W + MT - 1) / MT, tiles = tiles_of(H, W);
    double *ws = (double *)workspace;
    ps::for_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL(k_metrics_tiles<decltype(t)>, dim3(tiles, B), dim3(M_THREADS), 0, (hipStream_t)stream, a, b, mask, C, H, W,
                           tiles_x, ws);
    });
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_metrics_finish, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const double *)ws, B, tiles, C, H, W,
                       mask != nullptr, out);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
