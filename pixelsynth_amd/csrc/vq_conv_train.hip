// vq_conv_train.hip -- what makes the VQ-VAE's convolutions differentiable around the matrix products that exist already, for gfx950
// (MI355X), fp32 throughout, behind the C ABI of include/pixelsynth_vq_conv_train.h (libpixelsynth_vq_conv_train.so, beside
// libpixelsynth_hip.so whose set of exports it leaves as it is).
//
//   k_relu_pack         relu(x) or x, as it lies or as the 2 x 2 blocks conv_f16x3.hip reads for an s2d layer: the operand of a
//                       grad-weight GEMM, rebuilt in the backward pass from the saved raw input.  16 bytes per lane, one read, one write.
//   k_gate              unscale, + the skip's gradient, the ReLU's mask, in place: one pass where three would run.
//   k_fold              the 16 live of the 36 (block, sub-position) pairs of a 3 x 3 block weight's gradient, as the 4 x 4 weight's.
//   k_ends_grad_weight  the 64 x 48 sums over all pixels of the two 3-channel ends: a workgroup takes one image channel (16 taps) of one
//                       part of the pixels; its 16 groups of 16 lanes take the part's pixels in turn, a lane four wide channels, 16
//                       float4 accumulators per thread; the groups are added through LDS in ascending order and k_ends_sum_parts
//                       adds the parts.  The image values come through the L1 (16 floats per pixel, the same for the 16 lanes of a
//                       pixel); the wide tensor is read once per image channel.  The bias sums ride along in fp64.
//   k_head_grad_input   Conv2d(3, 64, 4, 2, 1) of the image's gradient on the fp32 matrix pipe, vq_ends.hip's stem with a plain NHWC
//                       output, no bias and the ReLU's mask: a wave takes 16 positions of a row, K = 48 = 12 MFMA steps.
// The order of every sum is in the header; tests/_vq_conv_train_ref.py restates it.  No atomics anywhere.
#include "ps_common.h"

#include <algorithm>

#include "../../include/pixelsynth_vq_conv_train.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int GROUPS = PS_VQ_CONV_TRAIN_GROUPS, LANES = THREADS / GROUPS;      // pixel groups of a workgroup; lanes per pixel (4 channels each)
static_assert(LANES * 4 == 64, "a pixel's 64 wide channels lie across its lanes");
constexpr int TAPS = 16, NW = 64 * 3 * TAPS;                                  // taps of an image channel; elements of an end's weight
constexpr size_t SLAB = NW + 2 * 64;                                            // floats of a part's slab: the sums, then 64 doubles of bias sums

using ps::aligned16;

unsigned grid_for(size_t total) { return (unsigned)std::min<size_t>((total + THREADS - 1) / THREADS, 256 * 32); }

// ---- the ReLU / pack pass ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_relu_pack(const f32x4 *__restrict__ x, size_t total4, int W, int C4, int relu, int s2d,
                                                      f32x4 *__restrict__ out)
{
    for (size_t e = (size_t)blockIdx.x * THREADS + threadIdx.x; e < total4; e += (size_t)gridDim.x * THREADS) {
        size_t src = e;
        if (s2d) {      // e = ((row of blocks * (W / 2) + xb) * 4 + q) * C4 + c4; the block row r lies at the pixel rows 2 r, 2 r + 1
            const size_t c4 = e % C4, rest = e / C4, q = rest & 3, xb = (rest >> 2) % (W / 2), r = (rest >> 2) / (W / 2);
            src = ((2 * r + (q >> 1)) * W + 2 * xb + (q & 1)) * C4 + c4;
        }
        const f32x4 v = x[src];
        out[e] = relu ? ps::relu_keep_nan(v) : v;
    }
}

// ---- the gate pass ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_gate(f32x4 *__restrict__ gx, const f32x4 *__restrict__ x, const f32x4 *__restrict__ skip,
                                                 const float *__restrict__ scale2, size_t total4)
{
    const float inv = scale2 ? scale2[1] : 1.0f;
    for (size_t e = (size_t)blockIdx.x * THREADS + threadIdx.x; e < total4; e += (size_t)gridDim.x * THREADS) {
        f32x4 v = gx[e];
        if (scale2) v = v * inv;
        if (skip) v = v + skip[e];
        if (x) {
            const f32x4 m = x[e];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = m[r] > 0.0f ? v[r] : 0.0f;
        }
        gx[e] = v;
    }
}

// ---- the fold pass -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_fold(const float *__restrict__ g, int Co, int Ci, int transposed, float *__restrict__ out)
{
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= Co * Ci * 16) return;
    const int kx = e & 3, ky = (e >> 2) & 3, second = (e >> 4) % (transposed ? Co : Ci), first = (e >> 4) / (transposed ? Co : Ci);
    const int sub = ((ky & 1) ^ 1) * 2 + ((kx & 1) ^ 1);                           // SY = {1, 0, 1, 0}
    size_t src;
    if (!transposed) {      // first = o, second = c;  BY = {0, 1, 1, 2} = (k + 1) / 2
        src = (((size_t)first * 3 + (ky + 1) / 2) * 3 + (kx + 1) / 2) * (4 * (size_t)Ci) + (size_t)sub * Ci + second;
    } else {                // first = c, second = o;  DY = {2, 1, 1, 0} = 2 - (k + 1) / 2
        src = ((((size_t)sub * Co + second) * 3 + (2 - (ky + 1) / 2)) * 3 + (2 - (kx + 1) / 2)) * (size_t)Ci + first;
    }
    out[e] = g[src];
}

// ---- the ends' weight and bias gradient -----------------------------------------------------------------------------------------------
struct Plan {
    size_t npix, part_pix, bytes;
    int parts;
};

inline bool pixels_ok(long long P) { return P >= 1 && P < ((long long)1 << 31); }

// The split of the pixels: a function of their number alone (the header's formula)
inline Plan plan_of(size_t npix)
{
    Plan p;
    p.npix = npix;
    const size_t steps = (npix + GROUPS - 1) / GROUPS;
    p.part_pix = std::max<size_t>(PS_VQ_CONV_TRAIN_MIN_PART, GROUPS * ((steps + PS_VQ_CONV_TRAIN_MAX_PARTS - 1) / PS_VQ_CONV_TRAIN_MAX_PARTS));
    p.parts = (int)((npix + p.part_pix - 1) / p.part_pix);
    p.bytes = ps::align_up((size_t)p.parts * SLAB * sizeof(float), 256);
    return p;
}

struct EgArgs {
    const float *img, *wide;
    int H, W, Hh, Wh, blocked;      // the image's sides; the wide tensor's (half of them)
    unsigned npix, part_pix;
    float *slab;
};

__device__ __forceinline__ f32x4 fma4(float s, f32x4 v, f32x4 acc)
{
    const f32x4 ss = {s, s, s, s};
    return __builtin_elementwise_fma(ss, v, acc);
}

__global__ __launch_bounds__(THREADS) void k_ends_grad_weight(EgArgs a)
{
    constexpr int CHUNK = 4;
    __shared__ f32x4 sRed[CHUNK][THREADS];      // (16 KB; the bias's 256 x 4 doubles take the first half of it afterwards)
    const int tid = threadIdx.x, lane = tid & (LANES - 1), grp = tid / LANES, c = blockIdx.x;
    const int H = a.H, W = a.W, Hh = a.Hh, Wh = a.Wh;
    const unsigned lo = blockIdx.y * a.part_pix, hi = (unsigned)std::min<size_t>(a.npix, (size_t)lo + a.part_pix);
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 acc[TAPS];
    double bs[4] = {0.0, 0.0, 0.0, 0.0};        // the bias's sums: fp64 all the way, rounded once by k_ends_sum_parts
#pragma unroll
    for (int i = 0; i < TAPS; ++i) acc[i] = zero;
    for (unsigned p = lo + grp; p < hi; p += GROUPS) {
        const int x = (int)(p % (unsigned)Wh), y = (int)((p / (unsigned)Wh) % (unsigned)Hh), b = (int)(p / ((unsigned)Wh * (unsigned)Hh));
        f32x4 wv;
        if (a.blocked) {
            wv = *(const f32x4 *)(a.wide + ((((size_t)b * (Hh / 2) + (y >> 1)) * (Wh / 2) + (x >> 1)) * 4 + (y & 1) * 2 + (x & 1)) * 64 + 4 * lane);
        } else {
            wv = ps::relu_keep_nan(*(const f32x4 *)(a.wide + (size_t)p * 64 + 4 * lane));
        }
        const float *plane = a.img + ((size_t)b * 3 + c) * H * W;
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
            const int iy = 2 * y - 1 + ky;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) {
                const int ix = 2 * x - 1 + kx;
                if (ix < 0 || ix >= W) continue;
                acc[ky * 4 + kx] = fma4(plane[(size_t)iy * W + ix], wv, acc[ky * 4 + kx]);
            }
        }
        if (a.blocked) {
            if (c == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) bs[r] += (double)wv[r];
            }
        } else if (lane == 0) {      // the image's own sum: the four pixels this position owns (they always lie inside the frame)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) bs[0] += (double)plane[(size_t)(2 * y + j) * W + 2 * x + i];
        }
    }

    // the groups in ascending order, CHUNK accumulators at a time: thread (i, lane) of the first CHUNK * LANES adds accumulator a0 + i
    float *dst = a.slab + (size_t)blockIdx.y * SLAB;
#pragma unroll
    for (int a0 = 0; a0 < TAPS; a0 += CHUNK) {
#pragma unroll
        for (int i = 0; i < CHUNK; ++i) sRed[i][tid] = acc[a0 + i];
        __syncthreads();
        const int i = tid / LANES;
        if (tid < CHUNK * LANES) {
            f32x4 v = sRed[i][lane];
            for (int q = 1; q < GROUPS; ++q) v = v + sRed[i][q * LANES + lane];
            *(f32x4 *)(dst + (size_t)(c * TAPS + a0 + i) * 64 + 4 * lane) = v;       // slab [c][tap][o]
        }
        __syncthreads();
    }
    // the bias's slot follows: 64 doubles.  The stem's: the wide sums of channel block 0; the head's: slot c, lane 0's sums
    if (a.blocked && c != 0) return;      // (uniform)
    double *sB = (double *)&sRed[0][0], *dstb = (double *)(dst + NW);
#pragma unroll
    for (int r = 0; r < 4; ++r) sB[tid * 4 + r] = bs[r];
    __syncthreads();
    if (a.blocked) {
        if (tid < LANES) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double v = sB[lane * 4 + r];
                for (int q = 1; q < GROUPS; ++q) v += sB[(q * LANES + lane) * 4 + r];
                dstb[4 * lane + r] = v;
            }
        }
    } else if (tid == 0) {
        double v = sB[0];
        for (int q = 1; q < GROUPS; ++q) v += sB[(q * LANES) * 4];
        dstb[c] = v;
    }
}

// grad_weight[o][c][tap] = slab[0][c][tap][o] + slab[1][c][tap][o] + ... in ascending part; the nb sums of the bias likewise in fp64,
// rounded to fp32 once
__global__ __launch_bounds__(THREADS) void k_ends_sum_parts(const float *__restrict__ slab, int parts, int nb, float *__restrict__ out_w,
                                                           float *__restrict__ out_b)
{
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e < NW) {
        const int o = e / (3 * TAPS), ct = e % (3 * TAPS);
        float v = slab[(size_t)ct * 64 + o];
#pragma unroll 16      // (the loads of 16 parts in flight; the adds stay in ascending order)
        for (int p = 1; p < parts; ++p) v = v + slab[(size_t)p * SLAB + (size_t)ct * 64 + o];
        out_w[e] = v;
    } else if (e - NW < nb) {
        double v = ((const double *)(slab + NW))[e - NW];
#pragma unroll 16
        for (int p = 1; p < parts; ++p) v += ((const double *)(slab + (size_t)p * SLAB + NW))[e - NW];
        out_b[e - NW] = (float)v;
    }
}

// ---- the head's input gradient --------------------------------------------------------------------------------------------------------
constexpr int HG_WAVES = 4;

struct HgArgs {
    const float *g, *wt, *h;     // (B, 3, 2 Hh, 2 Wh); (64, 3, 4, 4); (B, Hh, Wh, 64)
    float *gh;                   // (B, Hh, Wh, 64)
    int B, Hh, Wh;
};

__global__ __launch_bounds__(64 * HG_WAVES) void k_head_grad_input(HgArgs a)
{
    __shared__ float sW[4 * 12 * 64];        // [output tile t][step j][lane (o i, kk)] = wt[16 t + i][4 j + kk]  (k = c * 16 + ky * 4 + kx)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, kk = lane >> 4;
    for (int e = tid; e < 4 * 12 * 64; e += 64 * HG_WAVES) {
        const int l = e & 63, j = (e >> 6) % 12, t = (e >> 6) / 12;
        sW[e] = a.wt[(size_t)(t * 16 + (l & 15)) * 48 + 4 * j + (l >> 4)];
    }
    __syncthreads();
    const int Hh = a.Hh, Wh = a.Wh, H = 2 * Hh, W = 2 * Wh, tiles_row = Wh / 16;
    const size_t ntiles = (size_t)a.B * Hh * tiles_row;
    for (size_t tile = (size_t)blockIdx.x * HG_WAVES + wave; tile < ntiles; tile += (size_t)gridDim.x * HG_WAVES) {
        const int xg = (int)(tile % tiles_row);
        const size_t rest = tile / tiles_row;
        const int y = (int)(rest % Hh), b = (int)(rest / Hh), x = 16 * xg + i;      // this lane's position
        const int ix = 2 * x - 1 + kk;
        const float *img = a.g + (size_t)b * 3 * H * W;
        float v[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            const int c = j >> 2, iy = 2 * y - 1 + (j & 3);
            v[j] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? img[((size_t)c * H + iy) * W + ix] : 0.0f;
        }
        const size_t at = (((size_t)b * Hh + y) * Wh + x) * 64 + 4 * kk;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 12; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(sW[(t * 12 + j) * 64 + lane], v[j], acc, 0, 0, 0);
            const f32x4 m = *(const f32x4 *)(a.h + at + 16 * t);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = m[r] > 0.0f ? acc[r] : 0.0f;
            *(f32x4 *)(a.gh + at + 16 * t) = acc;
        }
    }
}

}  // namespace

extern "C" {

const char *ps_vq_conv_train_last_error(void) { return ps::last_error_ref().c_str(); }

int ps_vq_conv_train_parts(long long P) { return pixels_ok(P) ? plan_of((size_t)P).parts : 0; }

size_t ps_vq_conv_train_workspace_bytes(long long P) { return pixels_ok(P) ? plan_of((size_t)P).bytes : 0; }

int ps_vq_relu_pack_f32(const float *x, int B, int H, int W, int C, int relu, int s2d, float *out, void *stream)
{
    PS_REQUIRE(x && out && x != out, "vq_relu_pack: null pointer, or out is x");
    PS_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && (size_t)B * H * W * (size_t)C < ((size_t)1 << 33),
               "vq_relu_pack: C a multiple of 4 and B H W C < 2^33 required (B = %d, H = %d, W = %d, C = %d)", B, H, W, C);
    PS_REQUIRE(!s2d || (H % 2 == 0 && W % 2 == 0), "vq_relu_pack: even sides required for s2d (H = %d, W = %d)", H, W);
    PS_REQUIRE(aligned16(x) && aligned16(out), "vq_relu_pack: x and out must be aligned to 16 bytes");
    const size_t total4 = (size_t)B * H * W * (C / 4);
    hipLaunchKernelGGL(k_relu_pack, dim3(grid_for(total4)), dim3(THREADS), 0, (hipStream_t)stream, (const f32x4 *)x, total4, W, C / 4, relu != 0,
                       s2d != 0, (f32x4 *)out);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_vq_gate_f32(float *gx, const float *x, const float *skip, const float *scale2, size_t n, void *stream)
{
    PS_REQUIRE(gx, "vq_gate: null pointer");
    PS_REQUIRE(n > 0 && n % 4 == 0, "vq_gate: n a positive multiple of 4 required (n = %zu)", n);
    PS_REQUIRE(aligned16(gx) && aligned16(x) && aligned16(skip), "vq_gate: gx, x and skip must be aligned to 16 bytes");
    PS_REQUIRE(gx != x && gx != skip, "vq_gate: gx is x or skip");
    hipLaunchKernelGGL(k_gate, dim3(grid_for(n / 4)), dim3(THREADS), 0, (hipStream_t)stream, (f32x4 *)gx, (const f32x4 *)x, (const f32x4 *)skip,
                       scale2, n / 4);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_vq_fold_f32(const float *g, int Co, int Ci, int transposed, float *out, void *stream)
{
    PS_REQUIRE(g && out && g != out, "vq_fold: null pointer, or out is g");
    PS_REQUIRE(Co > 0 && Ci > 0 && (size_t)Co * Ci * 16 < ((size_t)1 << 31), "vq_fold: Co Ci 16 < 2^31 required (Co = %d, Ci = %d)", Co, Ci);
    hipLaunchKernelGGL(k_fold, dim3((Co * Ci * 16 + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream, g, Co, Ci, transposed != 0, out);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_vq_ends_grad_weight_f32(const float *img, const float *wide, int B, int H, int W, int blocked, float *grad_weight, float *grad_bias,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(img && wide && grad_weight, "vq_ends_grad_weight: null pointer");
    PS_REQUIRE(B > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && (!blocked || (H % 4 == 0 && W % 4 == 0)) &&
                   pixels_ok((long long)B * (H / 2) * (W / 2)),
               "vq_ends_grad_weight: even sides (multiples of 4 for the stem) and B H W / 4 < 2^31 required (B = %d, H = %d, W = %d)", B, H, W);
    PS_REQUIRE(aligned16(wide) && aligned16(workspace), "vq_ends_grad_weight: wide and the workspace must be aligned to 16 bytes");
    const Plan p = plan_of((size_t)B * (H / 2) * (W / 2));
    PS_REQUIRE(workspace, "vq_ends_grad_weight: null pointer (workspace)");
    PS_REQUIRE(workspace_bytes >= p.bytes, "vq_ends_grad_weight: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream;
    EgArgs a{img, wide, H, W, H / 2, W / 2, blocked != 0, (unsigned)p.npix, (unsigned)p.part_pix, (float *)workspace};
    hipLaunchKernelGGL(k_ends_grad_weight, dim3(3, p.parts), dim3(THREADS), 0, st, a);
    PS_LAUNCH_CHECK();
    const int nb = grad_bias ? (blocked ? 64 : 3) : 0;
    hipLaunchKernelGGL(k_ends_sum_parts, dim3((NW + nb + THREADS - 1) / THREADS), dim3(THREADS), 0, st, (const float *)workspace, p.parts, nb,
                       grad_weight, grad_bias);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_vq_head_grad_input_f32(const float *g_img, const float *wt, const float *h, int B, int Hh, int Wh, float *gh, void *stream)
{
    PS_REQUIRE(g_img && wt && h && gh, "vq_head_grad_input: null pointer");
    PS_REQUIRE(B > 0 && Hh > 0 && Wh > 0 && Wh % 16 == 0, "vq_head_grad_input: Wh a multiple of 16 required (Wh = %d)", Wh);
    PS_REQUIRE(aligned16(h) && aligned16(gh), "vq_head_grad_input: h and gh must be aligned to 16 bytes");
    HgArgs a{g_img, wt, h, gh, B, Hh, Wh};
    const size_t ntiles = (size_t)B * Hh * (Wh / 16);
    hipLaunchKernelGGL(k_head_grad_input, dim3((unsigned)std::min<size_t>((ntiles + HG_WAVES - 1) / HG_WAVES, 256 * 8)), dim3(64 * HG_WAVES), 0,
                       (hipStream_t)stream, a);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
