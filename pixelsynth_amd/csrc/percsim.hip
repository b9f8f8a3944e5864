// percsim.hip -- the glue of PercSim, the VGG16 perceptual similarity of image pairs (the reference's models/networks/
// pretrained_networks.py:11-93, :199-240: normalize_tensor, cos_sim, PNet, vgg16), for gfx950 (MI355X).  The 13 convolutions run on
// the existing split-fp16 kernels (conv_thin.hip for the 3 -> 64 stem, conv_f16x3.hip for the rest, ReLU applied on the way in, bias
// on the way out); what lies between them is here, so no standalone ReLU or max-pool pass is made:
//
//   k_percsim_input   one thread per pixel of an image pair: (img1, img2) (B, 3, H, W) fp32 or uint8 read through element strides ->
//                     out0, out1 (B, H, W, 4) fp32 NHWC, channel 3 zero, with the reference's fp32 operations in its order:
//                     u = x / 255 (uint8), u * m or u * (1 - m) (the masked variants), t = u * 2 - 1, (t - shift_c) / scale_c.
//   k_percsim_tap     one workgroup per (tile of 16 quads -- 2 x 2 pixel blocks --, pair); 16 lanes per quad, a lane owns 4 channels
//                     of every 64.  Reads the layer's pre-ReLU map y (2P, H, W, C) once (16-byte loads), the ReLU applied on the read:
//                     per pixel sum_c r0 r1, sum_c r0^2, sum_c r1^2 (fp32, fixed order, a fixed xor-butterfly over the 16 lanes),
//                     then dot / ((|r0| + 1e-10)(|r1| + 1e-10)) in fp64 -- cos_sim of the normalised maps without forming them.  The
//                     tile's 64 terms are added in a fixed order (fp64) and written to the workspace.  With `pooled`, the same read
//                     writes the 2 x 2 stride-2 max-pool of the PRE-ReLU map of both images: the next slice's input (its first
//                     convolution applies the ReLU, relu(max(y)) = max(relu(y))).  No atomics.  A NaN in y stays one, as in torch.relu
//                     and F.max_pool2d (ps::relu_keep_nan, ps::max4_keep_nan): in the pair's sums and in the pooled window that holds it.
//   k_percsim_finish  one workgroup per pair: per layer the tile sums (fp64, a fixed strided order and a fixed tree), 1 - mean, and
//                     the sum of the five.  A pair's numbers depend neither on its place in the batch nor on the batch's size.
//
// Workspace: [layer][pair][tile] doubles, tiles_l = (H_l / 2)(W_l / 2) / 16, H_l = H >> l.
#include "ps_image.h"
#include "../../include/pixelsynth_percsim.h"

#include <cmath>

namespace {

constexpr int T_THREADS = 256;           // 16 quads x 16 lanes
constexpr int T_QUADS = 16;              // quads per tile
constexpr int P_LAYERS = 5;              // relu1_2 .. relu5_3

enum { MODE_PLAIN = 0, MODE_VIS = 1, MODE_INVIS = 2, MODE_RAW = 3 };

using ps::c_pnet_scale;
using ps::c_pnet_shift;
using ps::f32x4;
using ps::Img;
using ps::max4_keep_nan;
using ps::to_unit;

template <typename T>
__global__ __launch_bounds__(256) void k_percsim_input(Img a, Img b, const float *__restrict__ mask, int mode, int H, int W,
                                                       f32x4 *__restrict__ out0, f32x4 *__restrict__ out1)
{
    const int pix = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
    if (pix >= H * W) return;
    const int h = pix / W, w = pix - h * W;
    float m = 1.0f;
    if (mode == MODE_VIS || mode == MODE_INVIS) {
        m = mask[(long long)img * H * W + pix];
        if (mode == MODE_INVIS) m = 1.0f - m;           // calc_errors_quality.py:38-47: mask = 1 - mask, then image * mask
    }
    auto one = [&](const Img &im, f32x4 *__restrict__ dst) {
        const T *p = (const T *)im.p + (long long)img * im.sB + (long long)h * im.sH + (long long)w * im.sW;
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float t = to_unit<T>(p[c * im.sC]);
            if (mode != MODE_RAW) {
                if (mode != MODE_PLAIN) t = t * m;
                t = t * 2.0f - 1.0f;                     // evaluation/metrics.py:27-31 (the unit is built without FP contraction)
            }
            o[c] = (t - c_pnet_shift[c]) / c_pnet_scale[c];
        }
        dst[(long long)img * H * W + pix] = o;
    };
    one(a, out0);
    one(b, out1);
}

template <bool POOL>
__global__ __launch_bounds__(T_THREADS) void k_percsim_tap(const f32x4 *__restrict__ y, int P, int H, int W, int C, int tiles,
                                                           f32x4 *__restrict__ pooled, double *__restrict__ part)
{
    __shared__ double red[T_QUADS];
    const int tid = threadIdx.x, slot = tid >> 4, l = tid & 15;
    const int tile = blockIdx.x, pair = blockIdx.y;
    const int Wq = W >> 1, q = tile * T_QUADS + slot, qy = q / Wq, qx = q - qy * Wq;
    const int C4 = C >> 2;
    // float4 offsets of the quad's four pixels in image `pair` and image `P + pair`
    const size_t img_px = (size_t)H * W;
    size_t off0[4], off1[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const size_t px = (size_t)(2 * qy + (p >> 1)) * W + 2 * qx + (p & 1);
        off0[p] = ((size_t)pair * img_px + px) * C4;
        off1[p] = ((size_t)(P + pair) * img_px + px) * C4;
    }
    const size_t pq = (size_t)(H >> 1) * Wq;
    const size_t poff0 = ((size_t)pair * pq + q) * C4, poff1 = ((size_t)(P + pair) * pq + q) * C4;
    float dot[4] = {0.f, 0.f, 0.f, 0.f}, n0[4] = {0.f, 0.f, 0.f, 0.f}, n1[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = l; c < C4; c += 16) {
        f32x4 v0[4], v1[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            v0[p] = y[off0[p] + c];
            v1[p] = y[off1[p] + c];
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const f32x4 r0 = ps::relu_keep_nan(v0[p]), r1 = ps::relu_keep_nan(v1[p]);   // (a NaN reaches the pair's sums, as torch's)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                dot[p] += r0[j] * r1[j];
                n0[p] += r0[j] * r0[j];
                n1[p] += r1[j] * r1[j];
            }
        }
        if (POOL) {
            pooled[poff0 + c] = max4_keep_nan(v0[0], v0[1], v0[2], v0[3]);
            pooled[poff1 + c] = max4_keep_nan(v1[0], v1[1], v1[2], v1[3]);
        }
    }
    // the 16 lanes of a quad: a fixed butterfly (every lane ends with the same, order-fixed sums)
#pragma unroll
    for (int s = 8; s > 0; s >>= 1)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            dot[p] += __shfl_xor(dot[p], s, 16);
            n0[p] += __shfl_xor(n0[p], s, 16);
            n1[p] += __shfl_xor(n1[p], s, 16);
        }
    double term = 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p)
        term += (double)dot[p] / ((sqrt((double)n0[p]) + 1e-10) * (sqrt((double)n1[p]) + 1e-10));
    if (l == 0) red[slot] = term;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < T_QUADS; ++k) s += red[k];
        part[(size_t)pair * tiles + tile] = s;
    }
}

int tiles_of(int H, int W, int layer) { return ((H >> layer) / 2) * ((W >> layer) / 2) / T_QUADS; }

size_t layer_offset(int P, int H, int W, int layer)   // doubles before `layer`'s block
{
    size_t o = 0;
    for (int k = 0; k < layer; ++k) o += (size_t)P * tiles_of(H, W, k);
    return o;
}

__global__ __launch_bounds__(64) void k_percsim_finish(const double *__restrict__ ws, int P, int H, int W, float *__restrict__ layers,
                                                       float *__restrict__ total)
{
    __shared__ double red[64];
    const int pair = blockIdx.x, l = threadIdx.x;
    const double *blk = ws;
    double tot = 0.0;
    for (int k = 0; k < P_LAYERS; ++k) {
        const int Hl = H >> k, Wl = W >> k, tiles = (Hl / 2) * (Wl / 2) / T_QUADS;
        const double *t = blk + (size_t)pair * tiles;
        double s = 0.0;
        for (int i = l; i < tiles; i += 64) s += t[i];
        red[l] = s;
        PS_BLOCK_TREE_SUM(red, l, 1, 64);
        const double score = 1.0 - red[0] / ((double)Hl * Wl);
        __syncthreads();                                  // before the next layer overwrites red
        if (l == 0) layers[(size_t)pair * P_LAYERS + k] = (float)score;
        tot += score;
        blk += (size_t)P * tiles;
    }
    if (l == 0) total[pair] = (float)tot;
}

}  // namespace

extern "C" {

const char *ps_percsim_last_error(void) { return ps::last_error_ref().c_str(); }

size_t ps_percsim_workspace_bytes(int P, int H, int W)
{
    if (P <= 0 || H <= 0 || W <= 0 || H % 128 || W % 128) return 0;
    return layer_offset(P, H, W, P_LAYERS) * sizeof(double);
}

int ps_percsim_input(const void *img1, const int64_t *strides1, const void *img2, const int64_t *strides2, int dtype, const float *mask,
                     int mode, int B, int H, int W, float *out0, float *out1, void *stream)
{
    PS_REQUIRE_IMAGES("percsim_input", img1 && img2 && strides1 && strides2 && out0 && out1, dtype, B, strides1, strides2);
    PS_REQUIRE(mode >= MODE_PLAIN && mode <= MODE_RAW, "percsim_input: mode %d", mode);
    PS_REQUIRE(mode != MODE_RAW || (dtype == PS_DTYPE_F32 && !mask), "percsim_input: PS_PERCSIM_RAW takes fp32 images and no mask");
    PS_REQUIRE((mode == MODE_VIS || mode == MODE_INVIS) == (mask != nullptr), "percsim_input: a mask goes with PS_PERCSIM_VIS / _INVIS");
    PS_REQUIRE(H >= 1 && W >= 1 && (size_t)H * W < ((size_t)1 << 31), "percsim_input: H = %d, W = %d", H, W);
    PS_REQUIRE(ps::aligned16(out0) && ps::aligned16(out1), "percsim_input: out0 / out1 must be 16-byte aligned");
    const Img a(img1, strides1), b(img2, strides2);
    const dim3 grid((unsigned)(((size_t)H * W + 255) / 256), B);
    ps::for_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL(k_percsim_input<decltype(t)>, grid, dim3(256), 0, (hipStream_t)stream, a, b, mask, mode, H, W, (f32x4 *)out0,
                           (f32x4 *)out1);
    });
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_percsim_tap(const float *y, int P, int H, int W, int layer, int C, float *pooled, void *workspace, size_t workspace_bytes,
                   void *stream)
{
    PS_REQUIRE(y && workspace, "percsim_tap: null pointer");
    PS_REQUIRE(P >= 1 && P <= 65535, "percsim_tap: 1 <= P <= 65535 required (P = %d)", P);
    PS_REQUIRE(H > 0 && W > 0 && H % 128 == 0 && W % 128 == 0, "percsim_tap: H and W multiples of 128 required (H = %d, W = %d)", H, W);
    PS_REQUIRE(layer >= 0 && layer < P_LAYERS, "percsim_tap: layer %d", layer);
    PS_REQUIRE(C > 0 && C % 64 == 0, "percsim_tap: C a multiple of 64 required (C = %d)", C);
    PS_REQUIRE(ps::aligned16(y) && ps::aligned16(pooled), "percsim_tap: y / pooled must be 16-byte aligned");
    const size_t need = ps_percsim_workspace_bytes(P, H, W);
    PS_REQUIRE(workspace_bytes >= need, "percsim_tap: workspace of %zu bytes required (got %zu)", need, workspace_bytes);
    const int Hl = H >> layer, Wl = W >> layer, tiles = tiles_of(H, W, layer);
    double *part = (double *)workspace + layer_offset(P, H, W, layer);
    if (pooled)
        hipLaunchKernelGGL(k_percsim_tap<true>, dim3(tiles, P), dim3(T_THREADS), 0, (hipStream_t)stream, (const f32x4 *)y, P, Hl, Wl, C,
                           tiles, (f32x4 *)pooled, part);
    else
        hipLaunchKernelGGL(k_percsim_tap<false>, dim3(tiles, P), dim3(T_THREADS), 0, (hipStream_t)stream, (const f32x4 *)y, P, Hl, Wl,
                           C, tiles, (f32x4 *)nullptr, part);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_percsim_finish(const void *workspace, size_t workspace_bytes, int P, int H, int W, float *layers, float *total, void *stream)
{
    PS_REQUIRE(workspace && layers && total, "percsim_finish: null pointer");
    PS_REQUIRE(P >= 1 && P <= 65535, "percsim_finish: 1 <= P <= 65535 required (P = %d)", P);
    PS_REQUIRE(H > 0 && W > 0 && H % 128 == 0 && W % 128 == 0, "percsim_finish: H and W multiples of 128 required (H = %d, W = %d)", H, W);
    const size_t need = ps_percsim_workspace_bytes(P, H, W);
    PS_REQUIRE(workspace_bytes >= need, "percsim_finish: workspace of %zu bytes required (got %zu)", need, workspace_bytes);
    hipLaunchKernelGGL(k_percsim_finish, dim3(P), dim3(64), 0, (hipStream_t)stream, (const double *)workspace, P, H, W, layers, total);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
