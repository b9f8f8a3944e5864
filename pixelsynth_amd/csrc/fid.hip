// fid.hip -- the passes of the FID network (Inception-v3 as pytorch_fid runs it, dims = 2048: networks/inception.py, fid.py) for gfx950
// (MI355X), on fp32 NHWC maps:
//
//   k_fid_input   one thread per output pixel: (B, 3, H, W) fp32 or uint8 read through element strides -> (B, 299, 299, 4), channel 3
//                 zero; torch's fp32 bilinear resize (align_corners = False) and 2 v - 1 in one pass, every product and sum of the
//                 formula below rounded once (the unit is built without FP contraction).  torch's own kernels round elsewhere
//                 (its CPU resize equals this one bit for bit on an exact 2 x downsample, and differs by the rounding of the
//                 source index on other sizes: tests/test_fid_conv_edges_gpu.py).
//   k_fid_conv    the project's general convolution: an implicit GEMM y (pixels, Co) = patches (pixels, K) . w^T (Co, K), K = KH KW Ci,
//                 on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation -- no split operands, no
//                 overflow guard), the epilogue max(acc + bias, 0) (BatchNorm folded into w and bias on the host; a NaN stays a
//                 NaN, as under torch.relu) written at a channel offset of a wider map: a block's branches land in its
//                 concatenated output, no concat pass exists.
//   k_fid_pool    the three 3 x 3 pools of the network and the final mean over the map, 4 channels per thread, the same
//                 channel-offset output.  A NaN in a window is the window's maximum, as under F.max_pool2d.
//
// The convolution.  K is walked in groups of 4 input channels of one tap (Ci is a multiple of 4: a group is one 16-byte load of one
// input pixel), 4 groups to a chunk (one MFMA k-step per element j of the groups), 4 chunks to a stage.  A workgroup of four waves
// owns T = 16 MT output channels and 4 x 16 NT pixels (MT x NT = 8 accumulator tiles a wave; T = 64 or 32, whichever pads Co less):
//   * weights: packed on the host in the order the kernel's LDS image has ([co block][stage][chunk][co tile][lane] x 4 floats,
//     zero-padded in Co and K), so a stage is 256 threads x MT contiguous 16-byte loads, kept in registers while the stage before it
//     computes, then written to the other half of a double-buffered LDS image: one barrier per stage.  A-fragments are one
//     conflict-free ds_read_b128 per tile and chunk.
//   * activations: lane (pixel i, group kk) loads x[pixel i + tap][4 c4 ..] of its NT pixels straight into the B registers (nobody else
//     needs them), one chunk ahead of the MFMAs that use them; a tap outside the map, a pixel past the end and a group past K load
//     nothing and count as zero.  The (tap, channel) of a lane's group advances by additions (no division in the loop).
//   * 32 MFMAs of 32 cycles per chunk and wave against MT LDS reads and NT global loads: the matrix pipe is what a wave waits for.
// Sum order of an output element, three levels so that the rounding error does not grow with K as one chain's would (one fp32 chain
// over K = 256 is already six times less accurate than the library's convolution): a chunk's 16 products are one fp32 fma chain from
// zero (j = 0 .. 3 outer, group kk = 0 .. 3 inner, k = 16 chunk + 4 kk + j); the chunks of four stages (16 chunks, ascending) are added
// into a middle sum; the middle sums are added in ascending order; the bias last.  The adds are VALU work under the MFMAs.  The order
// depends on nothing but the layer: bit-reproducible, batch-split invariant.
#include "ps_image.h"
#include "../../include/pixelsynth_fid.h"

namespace {

using ps::f32x4;
using ps::Img;
using ps::to_unit;

constexpr int FID_SIZE = 299;
constexpr int CV_THREADS = 256, CV_WAVES = 4, CV_STAGE_K = 64;

// torch.relu and F.max_pool2d hand a NaN on; v_max_f32 returns its other operand.  relu_nan: a compare and a select, NaN < 0 being
// false.  It has the bits of max(v, 0) for every other v but -0, which no sum that started at +0 ever is (k_fid_conv's do).
// MaxNan: the plain maximum of the values taken, and whether one of them was NaN (a compare into a scalar mask per value): the
// result is NaN then, the plain maximum's bits otherwise.
__device__ __forceinline__ float relu_nan(float v) { return v < 0.0f ? 0.0f : v; }
__device__ __forceinline__ f32x4 relu_nan(f32x4 v) { return (f32x4){relu_nan(v[0]), relu_nan(v[1]), relu_nan(v[2]), relu_nan(v[3])}; }

struct MaxNan {
    f32x4 m;
    bool nan[4];
    __device__ __forceinline__ explicit MaxNan(f32x4 v) : m(v), nan{v[0] != v[0], v[1] != v[1], v[2] != v[2], v[3] != v[3]} {}
    __device__ __forceinline__ void take(f32x4 v)
    {
        m = __builtin_elementwise_max(m, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) nan[c] |= v[c] != v[c];
    }
    __device__ __forceinline__ f32x4 result() const
    {
        const float q = __builtin_nanf("");
        return (f32x4){nan[0] ? q : m[0], nan[1] ? q : m[1], nan[2] ? q : m[2], nan[3] ? q : m[3]};
    }
};

template <typename T>
__global__ __launch_bounds__(256) void k_fid_input(Img im, int H, int W, float sh, float sw, f32x4 *__restrict__ out)
{
    const int pix = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
    if (pix >= FID_SIZE * FID_SIZE) return;
    const int oy = pix / FID_SIZE, ox = pix - oy * FID_SIZE;
    const T *p = (const T *)im.p + (long long)img * im.sB;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (H == FID_SIZE && W == FID_SIZE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = to_unit<T>(p[c * im.sC + oy * im.sH + ox * im.sW]) * 2.0f - 1.0f;
    } else {
        // aten's area_pixel_compute_source_index (align_corners = False, cubic = False) and upsample_bilinear2d's lambdas
        const float fy = fmaxf(sh * ((float)oy + 0.5f) - 0.5f, 0.0f), fx = fmaxf(sw * ((float)ox + 0.5f) - 0.5f, 0.0f);
        const int y0 = min((int)fy, H - 1), x0 = min((int)fx, W - 1);
        const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
        const float ly1 = fy - (float)y0, ly0 = 1.0f - ly1, lx1 = fx - (float)x0, lx0 = 1.0f - lx1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const T *q = p + c * im.sC;
            const float a = to_unit<T>(q[y0 * im.sH + x0 * im.sW]), b = to_unit<T>(q[y0 * im.sH + x1 * im.sW]);
            const float d = to_unit<T>(q[y1 * im.sH + x0 * im.sW]), e = to_unit<T>(q[y1 * im.sH + x1 * im.sW]);
            const float v = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * d + lx1 * e);
            o[c] = v * 2.0f - 1.0f;
        }
    }
    out[(long long)img * FID_SIZE * FID_SIZE + pix] = o;
}

struct ConvArgs {
    const float *x, *wp, *bias;
    float *y;                            // y + coff
    long long npix;                      // N Ho Wo
    int H, W, Ho, Wo, C4, KH, KW, stride, ph, pw, Co, ldx, ldy, S;   // C4 = Ci / 4; S = stages
};

template <int MT, int NT>
__global__ __launch_bounds__(CV_THREADS, 2) void k_fid_conv(ConvArgs a)
{
    constexpr int STAGE_F4 = 4 * MT * 64;                 // 16-byte words of a stage's weights
    __shared__ f32x4 sW[2][STAGE_F4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, kk = lane >> 4;
    const int cb = blockIdx.y, S = a.S;
    const f32x4 *wsrc = (const f32x4 *)a.wp + (size_t)cb * S * STAGE_F4 + tid;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    // this lane's NT pixels
    const long long p0 = ((long long)blockIdx.x * CV_WAVES + wave) * (16 * NT) + i;
    const float *base[NT];
    int hi0[NT], wi0[NT];
    bool pv[NT];
    const long long howo = (long long)a.Ho * a.Wo;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const long long p = p0 + 16 * n;
        pv[n] = p < a.npix;
        const long long pc = pv[n] ? p : 0;
        const long long img = pc / howo;
        const int r = (int)(pc - img * howo), ho = r / a.Wo, wo = r - ho * a.Wo;
        hi0[n] = ho * a.stride - a.ph;
        wi0[n] = wo * a.stride - a.pw;
        base[n] = a.x + (size_t)img * a.H * a.W * a.ldx;
    }
    // this lane's group of the current chunk: 4 channels c4 of tap (kh, kw); the next chunk's is 4 groups on
    int c4 = kk % a.C4, kw = (kk / a.C4) % a.KW, kh = (kk / a.C4) / a.KW;
    auto load_b = [&](f32x4 (&b)[NT]) {
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int hi = hi0[n] + kh, wi = wi0[n] + kw;
            const bool ok = pv[n] && kh < a.KH && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
            b[n] = zero;
            if (ok) b[n] = *(const f32x4 *)(base[n] + ((size_t)hi * a.W + wi) * a.ldx + 4 * c4);
        }
        c4 += 4;
        while (c4 >= a.C4) {
            c4 -= a.C4;
            if (++kw == a.KW) {
                kw = 0;
                ++kh;
            }
        }
    };

    // three levels of sums (header): a chunk's fma chain -> mid, the sum of up to 16 chunks -> acc
    f32x4 acc[MT][NT], mid[MT][NT], wreg[MT], bcur[NT], bnext[NT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[t][n] = mid[t][n] = zero;
#pragma unroll
    for (int n = 0; n < NT; ++n) bnext[n] = zero;
#pragma unroll
    for (int t = 0; t < MT; ++t) sW[0][t * CV_THREADS + tid] = wsrc[t * CV_THREADS];
    load_b(bcur);
    __syncthreads();
    for (int s = 0; s < S; ++s) {
        const bool more = s + 1 < S;
        if (more) {
#pragma unroll
            for (int t = 0; t < MT; ++t) wreg[t] = wsrc[(size_t)(s + 1) * STAGE_F4 + t * CV_THREADS];
        }
        const f32x4 *A = sW[s & 1] + lane;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c < 3 || more) load_b(bnext);
            f32x4 w4[MT];
#pragma unroll
            for (int t = 0; t < MT; ++t) w4[t] = A[(c * MT + t) * 64];
            f32x4 part[MT][NT];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < MT; ++t)
#pragma unroll
                    for (int n = 0; n < NT; ++n)
                        part[t][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[t][j], bcur[n][j], j ? part[t][n] : zero, 0, 0, 0);
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int n = 0; n < NT; ++n) mid[t][n] = mid[t][n] + part[t][n];
#pragma unroll
            for (int n = 0; n < NT; ++n) bcur[n] = bnext[n];
        }
        if ((s & 3) == 3 || !more) {
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    acc[t][n] = acc[t][n] + mid[t][n];
                    mid[t][n] = zero;
                }
        }
        if (more) {
#pragma unroll
            for (int t = 0; t < MT; ++t) sW[(s + 1) & 1][t * CV_THREADS + tid] = wreg[t];
        }
        __syncthreads();     // the other half was last read in stage s - 1, which every wave left at the barrier before this one
    }

    // lane (i, kk) of tile (t, n) holds y[pixel 16 n + i][16 t + 4 kk .. + 3]
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        if (!pv[n]) continue;
        float *row = a.y + (size_t)(p0 + 16 * n) * a.ldy;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int co = cb * (16 * MT) + 16 * t + 4 * kk;
            if (co + 3 < a.Co) {
                const f32x4 v = acc[t][n] + *(const f32x4 *)(a.bias + co);
                *(f32x4 *)(row + co) = relu_nan(v);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (co + r < a.Co) row[co + r] = relu_nan(acc[t][n][r] + a.bias[co + r]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_fid_pool(const float *__restrict__ x, int ldx, int mode, size_t total, int H, int W, int C4,
                                                  int Ho, int Wo, float *__restrict__ y, int ldy)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c4 = (int)(idx % C4);
    const size_t p = idx / C4;
    const int wo = (int)(p % Wo), ho = (int)((p / Wo) % Ho);
    const size_t n = p / ((size_t)Wo * Ho);
    const float *img = x + n * H * W * (size_t)ldx + 4 * c4;
    auto at = [&](int h, int w) { return *(const f32x4 *)(img + ((size_t)h * W + w) * ldx); };
    f32x4 o;
    if (mode == PS_FID_MEAN) {       // summed in fp64, rounded once: a map of any size costs one rounding
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int q = 0; q < H * W; ++q) {
            const f32x4 v = *(const f32x4 *)(img + (size_t)q * ldx);
            s0 += (double)v[0], s1 += (double)v[1], s2 += (double)v[2], s3 += (double)v[3];
        }
        const double hw = (double)H * W;
        o = (f32x4){(float)(s0 / hw), (float)(s1 / hw), (float)(s2 / hw), (float)(s3 / hw)};
    } else if (mode == PS_FID_MAX_S2) {
        MaxNan best(at(2 * ho, 2 * wo));
#pragma unroll
        for (int k = 1; k < 9; ++k) best.take(at(2 * ho + k / 3, 2 * wo + k % 3));
        o = best.result();
    } else {
        const int h0 = max(ho - 1, 0), h1 = min(ho + 1, H - 1), w0 = max(wo - 1, 0), w1 = min(wo + 1, W - 1);
        if (mode == PS_FID_MAX_S1) {
            MaxNan best(at(h0, w0));
            for (int h = h0; h <= h1; ++h)
                for (int w = w0; w <= w1; ++w) best.take(at(h, w));
            o = best.result();
        } else {
            o = (f32x4){0.f, 0.f, 0.f, 0.f};
            for (int h = h0; h <= h1; ++h)
                for (int w = w0; w <= w1; ++w) o = o + at(h, w);
            o = o / (float)((h1 - h0 + 1) * (w1 - w0 + 1));
        }
    }
    *(f32x4 *)(y + p * (size_t)ldy + 4 * c4) = o;
}

int conv_stages(int KH, int KW, int Ci) { return (KH * KW * Ci + CV_STAGE_K - 1) / CV_STAGE_K; }

template <int MT, int NT>
int launch_conv(const ConvArgs &a, hipStream_t st)
{
    const long long per = 16 * NT * CV_WAVES;
    const long long tiles = (a.npix + per - 1) / per;
    const int cbs = (a.Co + 16 * MT - 1) / (16 * MT);
    PS_REQUIRE(tiles <= 0x7fffffffLL && cbs <= 65535, "fid_conv: grid of %lld x %d workgroups", tiles, cbs);
    hipLaunchKernelGGL((k_fid_conv<MT, NT>), dim3((unsigned)tiles, cbs), dim3(CV_THREADS), 0, st, a);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // namespace

extern "C" {

const char *ps_fid_last_error(void) { return ps::last_error_ref().c_str(); }

int ps_fid_input(const void *img, const int64_t *strides, int dtype, int B, int H, int W, float *out, void *stream)
{
    PS_REQUIRE_IMAGES("fid_input", img && strides && out, dtype, B, strides, nullptr);
    PS_REQUIRE(H >= 1 && W >= 1 && (size_t)H * W < ((size_t)1 << 31), "fid_input: H = %d, W = %d", H, W);
    PS_REQUIRE(ps::aligned16(out), "fid_input: out must be 16-byte aligned");
    const Img im(img, strides);
    const float sh = (float)H / (float)FID_SIZE, sw = (float)W / (float)FID_SIZE;
    const dim3 grid((FID_SIZE * FID_SIZE + 255) / 256, B);
    ps::for_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL(k_fid_input<decltype(t)>, grid, dim3(256), 0, (hipStream_t)stream, im, H, W, sh, sw, (f32x4 *)out);
    });
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_fid_conv_takes(int KH, int KW, int stride, int ph, int pw, int Ci, int Co)
{
    return KH >= 1 && KH <= 7 && KW >= 1 && KW <= 7 && (stride == 1 || stride == 2) && ph >= 0 && ph < KH && pw >= 0 && pw < KW &&
           Ci >= 4 && Ci % 4 == 0 && Ci <= (1 << 20) && Co >= 1 && Co <= (1 << 20);
}

int ps_fid_conv_co_tile(int Co) { return Co > 0 && (Co + 31) / 32 * 32 < (Co + 63) / 64 * 64 ? 32 : 64; }

size_t ps_fid_conv_packed_floats(int KH, int KW, int Ci, int Co)
{
    if (!ps_fid_conv_takes(KH, KW, 1, 0, 0, Ci, Co)) return 0;
    const int T = ps_fid_conv_co_tile(Co);
    return (size_t)((Co + T - 1) / T) * T * conv_stages(KH, KW, Ci) * CV_STAGE_K;
}

int ps_fid_conv(const float *x, int ldx, const float *wp, size_t wp_floats, const float *bias, int N, int H, int W, int Ci, int KH, int KW,
                int stride, int ph, int pw, int Co, float *y, int ldy, int coff, void *stream)
{
    PS_REQUIRE(x && wp && bias && y, "fid_conv: null pointer");
    PS_REQUIRE(ps_fid_conv_takes(KH, KW, stride, ph, pw, Ci, Co),
               "fid_conv: 1 <= KH, KW <= 7, stride 1 or 2, 0 <= pad < kernel, Ci a multiple of 4 and Co >= 1 required (KH = %d, KW = %d, "
               "stride = %d, pad = (%d, %d), Ci = %d, Co = %d)", KH, KW, stride, ph, pw, Ci, Co);
    PS_REQUIRE(N >= 1 && H >= 1 && W >= 1 && H + 2 * ph >= KH && W + 2 * pw >= KW, "fid_conv: N = %d, H = %d, W = %d", N, H, W);
    PS_REQUIRE((size_t)H * W < ((size_t)1 << 31), "fid_conv: H = %d, W = %d", H, W);
    PS_REQUIRE(ldx >= Ci && ldx % 4 == 0, "fid_conv: ldx >= Ci and a multiple of 4 required (ldx = %d)", ldx);
    PS_REQUIRE(coff >= 0 && coff % 4 == 0 && ldy % 4 == 0 && ldy >= coff + Co,
               "fid_conv: coff and ldy multiples of 4, coff + Co <= ldy required (coff = %d, Co = %d, ldy = %d)", coff, Co, ldy);
    PS_REQUIRE(ps::aligned16(x) && ps::aligned16(wp) && ps::aligned16(y) && ps::aligned16(bias), "fid_conv: 16-byte aligned buffers required");
    const size_t need = ps_fid_conv_packed_floats(KH, KW, Ci, Co);
    PS_REQUIRE(wp_floats == need, "fid_conv: packed weights of %zu floats required (got %zu)", need, wp_floats);
    const int Ho = (H + 2 * ph - KH) / stride + 1, Wo = (W + 2 * pw - KW) / stride + 1;
    ConvArgs a{x, wp, bias, y + coff, (long long)N * Ho * Wo, H, W, Ho, Wo, Ci / 4, KH, KW, stride, ph, pw, Co, ldx, ldy,
               conv_stages(KH, KW, Ci)};
    return ps_fid_conv_co_tile(Co) == 32 ? launch_conv<2, 4>(a, (hipStream_t)stream) : launch_conv<4, 2>(a, (hipStream_t)stream);
}

int ps_fid_pool(const float *x, int ldx, int mode, int N, int H, int W, int C, float *y, int ldy, int coff, void *stream)
{
    PS_REQUIRE(x && y, "fid_pool: null pointer");
    PS_REQUIRE(mode >= PS_FID_MAX_S2 && mode <= PS_FID_MEAN, "fid_pool: mode %d", mode);
    PS_REQUIRE(N >= 1 && H >= 1 && W >= 1 && (size_t)H * W < ((size_t)1 << 31), "fid_pool: N = %d, H = %d, W = %d", N, H, W);
    PS_REQUIRE(mode != PS_FID_MAX_S2 || (H >= 3 && W >= 3), "fid_pool: PS_FID_MAX_S2 takes maps of 3 x 3 and more (H = %d, W = %d)", H, W);
    PS_REQUIRE(C >= 4 && C % 4 == 0, "fid_pool: C a multiple of 4 required (C = %d)", C);
    PS_REQUIRE(ldx >= C && ldx % 4 == 0, "fid_pool: ldx >= C and a multiple of 4 required (ldx = %d)", ldx);
    PS_REQUIRE(coff >= 0 && coff % 4 == 0 && ldy % 4 == 0 && ldy >= coff + C,
               "fid_pool: coff and ldy multiples of 4, coff + C <= ldy required (coff = %d, C = %d, ldy = %d)", coff, C, ldy);
    PS_REQUIRE(ps::aligned16(x) && ps::aligned16(y), "fid_pool: 16-byte aligned buffers required");
    const int Ho = mode == PS_FID_MEAN ? 1 : mode == PS_FID_MAX_S2 ? (H - 3) / 2 + 1 : H;
    const int Wo = mode == PS_FID_MEAN ? 1 : mode == PS_FID_MAX_S2 ? (W - 3) / 2 + 1 : W;
    const size_t total = (size_t)N * Ho * Wo * (C / 4);
    PS_REQUIRE((total + 255) / 256 <= 0x7fffffffULL, "fid_pool: %zu outputs", total);
    hipLaunchKernelGGL(k_fid_pool, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, mode, total, H, W,
                       C / 4, Ho, Wo, y + coff, ldy);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
