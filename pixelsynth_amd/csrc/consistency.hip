// consistency.hip -- the homography consistency score of two views (the reference's calc_errors_consistency_homography.py:66-105), for
// gfx950 (MI355X): both warps of every item, the masked comparison and, on request, PercSim's network input, in one pass.
//
//   k_consistency_tiles   one workgroup per (tile of 64 x 4 output pixels, direction, item), a thread per pixel.  The source position
//                         is OpenCV's warpPerspective with INTER_LINEAR and BORDER_CONSTANT 0, restated from the scalar path of
//                         WarpPerspectiveInvoker (modules/imgproc/src/imgwarp.cpp, OpenCV 4.x before the 4.11 warp rewrite) and
//                         remapBilinear of the same file: per block of bw0 columns (bh0 = min(16, H), bw0 = min(1024 / bh0, W)), with
//                         xb the block's first column and x1 = x - xb,
//                           X0 = M0 xb + M1 y + M2, Y0 = M3 xb + M4 y + M5, W0 = M6 xb + M7 y + M8      (fp64, left to right)
//                           W = W0 + M6 x1, W = W ? 32 / W : 0, X = rint(clamp((X0 + M0 x1) W)), Y likewise (clamp to int's range)
//                           column sat_short(X >> 5), fraction X & 31; rows likewise
//                         the 4 taps (0 outside the image) weighted by the fp32 bilinear table, v0 w0 + v1 w1 + v2 w2 + v3 w3 in fp32.
//                         The taps are gathered straight from global memory: a perspective map's footprint is not bounded, so no
//                         source tile is staged (near-identity maps read nearly contiguous rows, which the caches serve).
//                         Then the masked comparison in the reference's fp32 operations, and the tile's fp64 sums of m sum_c d^2 and
//                         of m, reduced in a fixed tree and written to the workspace.  No atomics.
//   k_consistency_finish  one thread per (item, direction): the tile sums in tile order (fp64), PSNR clamped at 100.
#include "ps_image.h"
#include "../../include/pixelsynth_consistency.h"

#include <climits>
#include <cmath>

namespace {

constexpr int TX = 64, TY = 4, C_THREADS = TX * TY;

using ps::c_pnet_scale;
using ps::c_pnet_shift;
using ps::f32x4;
using ps::Img;

// TF.to_tensor's value of an input element: fp32 as it is; a byte b as fl32(b / 255), the true division of float().div(255) on the
// host (not a multiply by the reciprocal), looked up in the workgroup's table of the 256 quotients (16 byte reads per pixel): this
// unit's variant of ps::to_unit
__device__ __forceinline__ float to_unit(float v, const float *) { return v; }
__device__ __forceinline__ float to_unit(uint8_t v, const float *quot) { return quot[v]; }
static_assert(C_THREADS == 256, "a thread per entry of the byte table");

// PNet's shift / scale (ps_image.h) are RGB constants, applied to the BGR-ordered channels as the reference does
// (calc_errors_consistency_homography.py:24-30 feeds cv2's channel order to PNet)

// std::max((double)INT_MIN, std::min((double)INT_MAX, v)) then saturate_cast<int> (round to nearest even)
__device__ __forceinline__ int cv_round_clamped(double v)
{
    const double hi = (double)INT_MAX, lo = (double)INT_MIN;
    v = (v < hi) ? v : hi;               // std::min(hi, v): NaN -> hi
    v = (lo < v) ? v : lo;               // std::max(lo, v)
    return (int)__builtin_rint(v);
}

__device__ __forceinline__ int sat_short(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

template <typename T, typename TM>
__global__ __launch_bounds__(C_THREADS) void k_consistency_tiles(Img v1, Img v2, const TM *__restrict__ mask1, const TM *__restrict__ mask2,
                                                                 const double *__restrict__ maps, int B, int H, int W, int bw0, int tiles_x,
                                                                 int pmode, f32x4 *__restrict__ pin, double *__restrict__ ws)
{
    __shared__ double red[2 * C_THREADS];
    __shared__ float quot[256];
    const int tid = threadIdx.x, tile = blockIdx.x, k = blockIdx.y, item = blockIdx.z;
    quot[tid] = (float)tid / 255.0f;
    __syncthreads();
    const int x = (tile % tiles_x) * TX + (tid & (TX - 1)), y = (tile / tiles_x) * TY + (tid >> 6);
    double s_d = 0.0, s_m = 0.0;
    if (x < W && y < H) {
        // direction 0: view 2 warped into frame 1, compared with view 1 under mask 1; direction 1 the other way round
        const Img &src = k == 0 ? v2 : v1, &ref = k == 0 ? v1 : v2;
        const TM *mk = k == 0 ? mask1 : mask2;
        const double *M = maps + ((size_t)item * 2 + k) * 9;
        const int xb = (x / bw0) * bw0, x1 = x - xb;
        const double X0 = M[0] * xb + M[1] * y + M[2], Y0 = M[3] * xb + M[4] * y + M[5], W0 = M[6] * xb + M[7] * y + M[8];
        double Wd = W0 + M[6] * x1;
        Wd = Wd != 0.0 ? 32.0 / Wd : 0.0;
        const int X = cv_round_clamped((X0 + M[0] * x1) * Wd), Y = cv_round_clamped((Y0 + M[3] * x1) * Wd);
        const int sx = sat_short(X >> 5), sy = sat_short(Y >> 5);
        // the 32 x 32 bilinear table (initInterTab2D): w[k1 2 + k2] = vy[k1] vx[k2], v = (1 - i / 32, i / 32), all exact in fp32
        const float fx = (float)(X & 31) * (1.0f / 32.0f), fy = (float)(Y & 31) * (1.0f / 32.0f);
        const float w[4] = {(1.0f - fy) * (1.0f - fx), (1.0f - fy) * fx, fy * (1.0f - fx), fy * fx};
        const bool in[4] = {sx >= 0 && sx < W && sy >= 0 && sy < H, sx + 1 >= 0 && sx + 1 < W && sy >= 0 && sy < H,
                            sx >= 0 && sx < W && sy + 1 >= 0 && sy + 1 < H, sx + 1 >= 0 && sx + 1 < W && sy + 1 >= 0 && sy + 1 < H};
        const T *ps = (const T *)src.p + (long long)item * src.sB;
        const T *pr = (const T *)ref.p + (long long)item * ref.sB + (long long)y * ref.sH + (long long)x * ref.sW;
        const float m = to_unit(mk[((size_t)item * H + y) * W + x], quot);
        f32x4 oa = {0.f, 0.f, 0.f, 0.f}, ob = {0.f, 0.f, 0.f, 0.f};
        double d2 = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {                   // BGR channel j = RGB channel 2 - j
            const long long c = (long long)(2 - j) * src.sC;
            float v[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const long long off = c + (long long)(sy + (t >> 1)) * src.sH + (long long)(sx + (t & 1)) * src.sW;
                v[t] = in[t] ? to_unit(ps[off], quot) * 255.0f : 0.0f;  // try = fl32(u * 255)
            }
            const float warped = v[0] * w[0] + v[1] * w[1] + v[2] * w[2] + v[3] * w[3];
            const float a = (warped * m) / 255.0f;                        // (im_out * m) / 255
            const float u = to_unit(pr[(long long)(2 - j) * ref.sC], quot);
            const float b = ((m * u) * 255.0f) / 255.0f;                   // outmask / 255
            const float d = a - b;
            d2 += (double)(d * d);
            if (pmode != PS_CONSISTENCY_NO_PERCSIM) {
                const float ta = a * 2.0f - 1.0f, tb = b * 2.0f - 1.0f;   // evaluation/metrics.py:27-31
                oa[j] = pmode == PS_CONSISTENCY_PERCSIM ? (ta - c_pnet_shift[j]) / c_pnet_scale[j] : ta;
                ob[j] = pmode == PS_CONSISTENCY_PERCSIM ? (tb - c_pnet_shift[j]) / c_pnet_scale[j] : tb;
            }
        }
        s_d = (double)m * d2;
        s_m = (double)m;
        if (pmode != PS_CONSISTENCY_NO_PERCSIM) {
            const size_t px = (size_t)y * W + x, img_px = (size_t)H * W, p = (size_t)item * 2 + k;
            pin[p * img_px + px] = oa;
            pin[((size_t)2 * B + p) * img_px + px] = ob;
        }
    }
    red[tid] = s_d;
    red[C_THREADS + tid] = s_m;
    PS_BLOCK_TREE_SUM(red, tid, 2, C_THREADS);
    if (tid < 2) ws[(((size_t)item * 2 + k) * gridDim.x + tile) * 2 + tid] = red[tid * C_THREADS];
}

__global__ __launch_bounds__(64) void k_consistency_finish(const double *__restrict__ ws, int B, int tiles, float *__restrict__ psnr)
{
    const int r = blockIdx.x * 64 + threadIdx.x;          // item * 2 + direction
    if (r >= 2 * B) return;
    double s_d = 0.0, s_m = 0.0;
    for (int t = 0; t < tiles; ++t) {
        s_d += ws[((size_t)r * tiles + t) * 2];
        s_m += ws[((size_t)r * tiles + t) * 2 + 1];
    }
    // evaluation/metrics.py:11-23 with the reference's literal 3; an empty mask gives 1 / 0 = inf, which the clamp turns into 100
    const float p = (float)(10.0 * log10(1.0 / (s_d / (3.0 * fmax(s_m, 1.0)))));
    psnr[r] = p > 100.0f ? 100.0f : p;                     // .clamp(max=100) (NaN stays NaN)
}

int tiles_of(int H, int W) { return ((W + TX - 1) / TX) * ((H + TY - 1) / TY); }

template <typename T, typename TM>
void launch(const Img &a, const Img &b, const void *m1, const void *m2, const double *maps, int B, int H, int W, int pmode, float *pin,
            double *ws, hipStream_t stream)
{
    int bh0 = H < 16 ? H : 16;                              // WarpPerspectiveInvoker's block shape
    int bw0 = 1024 / bh0 < W ? 1024 / bh0 : W;
    const int tiles_x = (W + TX - 1) / TX;
    hipLaunchKernelGGL((k_consistency_tiles<T, TM>), dim3(tiles_of(H, W), 2, B), dim3(C_THREADS), 0, stream, a, b, (const TM *)m1,
                       (const TM *)m2, maps, B, H, W, bw0, tiles_x, pmode, (f32x4 *)pin, ws);
}

}  // namespace

extern "C" {

const char *ps_consistency_last_error(void) { return ps::last_error_ref().c_str(); }

size_t ps_consistency_workspace_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * 2 * tiles_of(H, W) * 2 * sizeof(double);
}

int ps_consistency(const void *view1, const int64_t *strides1, const void *view2, const int64_t *strides2, int dtype, const void *mask1,
                   const void *mask2, int mask_dtype, const double *inv_maps, int B, int H, int W, int percsim_mode, float *percsim_in,
                   float *psnr, void *workspace, size_t workspace_bytes, void *stream)
{
    PS_REQUIRE_IMAGES("consistency", view1 && view2 && strides1 && strides2 && mask1 && mask2 && inv_maps && psnr, dtype, B, strides1,
                      strides2);
    PS_REQUIRE(mask_dtype == PS_DTYPE_F32 || mask_dtype == PS_DTYPE_U8,
               "consistency: mask_dtype must be PS_DTYPE_F32 or PS_DTYPE_U8 (got %d)", mask_dtype);
    PS_REQUIRE(H >= 1 && W >= 1 && H <= 32767 && W <= 32767, "consistency: 1 <= H, W <= 32767 required (H = %d, W = %d)", H, W);
    PS_REQUIRE(percsim_mode >= PS_CONSISTENCY_NO_PERCSIM && percsim_mode <= PS_CONSISTENCY_PERCSIM_RAW, "consistency: percsim_mode %d",
               percsim_mode);
    PS_REQUIRE((percsim_mode == PS_CONSISTENCY_NO_PERCSIM) == (percsim_in == nullptr),
               "consistency: percsim_in goes with PS_CONSISTENCY_PERCSIM / _PERCSIM_RAW");
    PS_REQUIRE(ps::aligned16(percsim_in), "consistency: percsim_in must be 16-byte aligned");
    const size_t need = ps_consistency_workspace_bytes(B, H, W);
    PS_REQUIRE(workspace && workspace_bytes >= need, "consistency: workspace of %zu bytes required (got %zu)", need, workspace_bytes);
    const Img a(view1, strides1), b(view2, strides2);
    double *ws = (double *)workspace;
    const hipStream_t s = (hipStream_t)stream;
    ps::for_dtype(dtype, [&](auto t) {
        ps::for_dtype(mask_dtype, [&](auto tm) {
            launch<decltype(t), decltype(tm)>(a, b, mask1, mask2, inv_maps, B, H, W, percsim_mode, percsim_in, ws, s);
        });
    });
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_consistency_finish, dim3((2 * B + 63) / 64), dim3(64), 0, s, (const double *)ws, B, tiles_of(H, W), psnr);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
