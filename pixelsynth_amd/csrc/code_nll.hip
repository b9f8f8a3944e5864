// code_nll.hip -- the likelihood the PixelCNN gives to GIVEN codes, for gfx950 (MI355X): per location the negative log-likelihood of the
// target code under softmax(logits / T), the entropy of that distribution and whether the target is its arg-max; per frame their fp64
// sums over the observed and the sampled locations.
//
// Behind the C ABI of include/pixelsynth_nll.h (libpixelsynth_nll.so, beside libpixelsynth_hip.so whose set of exports it leaves as it
// is).  The logits come in the two layouts the engine emits, each read the way that coalesces for it, each ONCE:
//   k_code_nll_chw   (F,512,L), what ps_pixelcnn_forward_f32 writes: one workgroup per 64 consecutive locations, lanes across the
//                    locations; its four waves hold a quarter of the classes each in registers (128 loads of 256 contiguous bytes per
//                    wave), find the maximum, exchange it through LDS, sum their exponentials, exchange those.
//   k_code_nll_lc    (F,L,512), out_logits of the AR runs: one wave per location, lane l holds classes 8l .. 8l+7 as draw_code
//                    (lmconv_device.h) holds them -- two 16-byte loads per lane --, butterflies across the lanes.
//   k_nll_frames     one workgroup per frame: the fp64 sums of the per-location outputs per group, thread t over locations t, t + 256,
//                    ... in that order, then a fixed pairwise tree in LDS.  No atomic; a frame's row depends on that frame alone.
//
// Numerics (the same in both kernels but for the order of the 512-term sums).  M = the largest logit; per class d = (x - M) / T and
// e = expf(d) in fp32: d is formed from the DIFFERENCE, so its error is relative to |d| -- a class that matters to the sum has a small
// |d|, and the magnitude of the logits does not enter --, and d <= 0 always: nothing overflows.  s = sum e, w = sum e d (a class with
// e = 0 adds 0, also where d is -inf), both added as TREES nine levels deep (eight classes, sixteen of those, four waves; or eight
// classes and a butterfly over the lanes): a term passes nine roundings, not 511.  Then in fp64, per location:
// nll = log s - (x_t - M) / T, entropy = log s - w / s, each rounded to fp32 once -- the magnitude of the logits enters the nll through
// that one rounding alone.  A NaN logit makes s NaN, and both results with it; the maximum and the arg-max skip it.  A target outside
// [0, 512) is never used as an index.
#include "ps_common.h"

#include <cmath>

#include "../../include/pixelsynth_nll.h"

namespace {

constexpr int NCLS = PS_NLL_CLASSES;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int CHW_LOCS = 64;                    // locations per workgroup of k_code_nll_chw
constexpr int CHW_CLS = NCLS / WAVES;           // classes per wave there
constexpr int LC_LOCS = WAVES;                  // locations per workgroup of k_code_nll_lc
constexpr int LC_CLS = NCLS / 64;               // classes per lane there
static_assert(LC_CLS == 8, "a lane of k_code_nll_lc loads two float4");

// (value, class) a before b: the larger value, the lower class among equal ones; a NaN is never larger
__device__ __forceinline__ bool ahead(float va, int ca, float vb, int cb) { return va > vb || (va == vb && ca < cb); }

// Eight classes: d = (x - M) / T, e = expf(d); s = sum e, w = sum e d (a class with e = 0 adds 0 to w whatever its d, a NaN stays one),
// each added as a tree three levels deep
__device__ __forceinline__ void terms8(const float *x, float M, float Tf, float &s, float &w)
{
    float e[8], p[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float d = (x[k] - M) / Tf;
        e[k] = expf(d);
        p[k] = e[k] > 0.0f ? e[k] * d : (e[k] != e[k] ? e[k] : 0.0f);
    }
    s = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
    w = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
}

// sixteen partial sums as a tree four levels deep
__device__ __forceinline__ float tree16(float (&v)[16])
{
#pragma unroll
    for (int n = 8; n > 0; n >>= 1)
#pragma unroll
        for (int c = 0; c < n; ++c) v[c] += v[c + n];
    return v[0];
}

// the per-location results from M, s = sum exp(d), w = sum exp(d) d, the arg-max and the target's logit xt (read only where `valid`)
__device__ __forceinline__ void finish(size_t at, bool valid, int t, float xt, float M, float s, float w, int arg, double T,
                                       float *__restrict__ nll, float *__restrict__ entropy, uint8_t *__restrict__ hit)
{
    const double ls = log((double)s);
    if (nll) nll[at] = valid ? (float)(ls - ((double)xt - (double)M) / T) : NAN;
    if (entropy) entropy[at] = (float)(ls - (double)w / (double)s);
    if (hit) hit[at] = valid && t == arg;
}

__global__ __launch_bounds__(THREADS) void k_code_nll_chw(const float *__restrict__ logits, const int32_t *__restrict__ targets, double T,
                                                          int L, float *__restrict__ nll, float *__restrict__ entropy,
                                                          uint8_t *__restrict__ hit)
{
    __shared__ float sh_v[WAVES][CHW_LOCS], sh_w[WAVES][CHW_LOCS];
    __shared__ int sh_c[WAVES][CHW_LOCS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.y;
    const int loc = blockIdx.x * CHW_LOCS + lane;
    const int q = loc < L ? loc : L - 1;        // a lane past the frame reads its last location and writes nothing
    const int c0 = wave * CHW_CLS;
    const float *p = logits + ((size_t)f * NCLS + c0) * (size_t)L + q;
    float x[CHW_CLS];
#pragma unroll
    for (int k = 0; k < CHW_CLS; ++k) x[k] = p[(size_t)k * L];
    float best = -INFINITY;
    int arg = c0;
#pragma unroll
    for (int k = 0; k < CHW_CLS; ++k)
        if (x[k] > best) { best = x[k]; arg = c0 + k; }
    sh_v[wave][lane] = best;
    sh_c[wave][lane] = arg;
    __syncthreads();
    float M = sh_v[0][lane];
    arg = sh_c[0][lane];
#pragma unroll
    for (int v = 1; v < WAVES; ++v)
        if (sh_v[v][lane] > M) { M = sh_v[v][lane]; arg = sh_c[v][lane]; }
    __syncthreads();                            // (sh_v is written again below)
    const float Tf = (float)T;
    float es[CHW_CLS / 8], ws[CHW_CLS / 8];
#pragma unroll
    for (int c = 0; c < CHW_CLS / 8; ++c) terms8(&x[c * 8], M, Tf, es[c], ws[c]);
    float s = tree16(es), w = tree16(ws);
    static_assert(CHW_CLS == 128, "sixteen sums of eight classes per wave");
    sh_v[wave][lane] = s;
    sh_w[wave][lane] = w;
    __syncthreads();
    if (wave != 0 || loc >= L) return;
    s = (sh_v[0][lane] + sh_v[1][lane]) + (sh_v[2][lane] + sh_v[3][lane]);
    w = (sh_w[0][lane] + sh_w[1][lane]) + (sh_w[2][lane] + sh_w[3][lane]);
    static_assert(WAVES == 4, "the two lines above add four partial sums");
    const size_t at = (size_t)f * L + loc;
    const int t = targets[at];
    const bool valid = (unsigned)t < (unsigned)NCLS;
    const float xt = valid ? logits[((size_t)f * NCLS + t) * (size_t)L + loc] : 0.0f;
    finish(at, valid, t, xt, M, s, w, arg, T, nll, entropy, hit);
}

__global__ __launch_bounds__(THREADS) void k_code_nll_lc(const float *__restrict__ logits, const int32_t *__restrict__ targets, double T,
                                                         int L, float *__restrict__ nll, float *__restrict__ entropy,
                                                         uint8_t *__restrict__ hit)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.y;
    const int loc = blockIdx.x * LC_LOCS + wave;
    if (loc >= L) return;                       // (whole waves; the kernel has no barrier)
    const size_t at = (size_t)f * L + loc;
    const float *row = logits + at * NCLS;
    const float4 lo = reinterpret_cast<const float4 *>(row)[lane * 2], hi = reinterpret_cast<const float4 *>(row)[lane * 2 + 1];
    const float x[LC_CLS] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    float M = -INFINITY;
    int arg = lane * LC_CLS;
#pragma unroll
    for (int k = 0; k < LC_CLS; ++k)
        if (x[k] > M) { M = x[k]; arg = lane * LC_CLS + k; }
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(M, off, 64);
        const int oc = __shfl_xor(arg, off, 64);
        if (ahead(ov, oc, M, arg)) { M = ov; arg = oc; }
    }
    const float Tf = (float)T;
    float s, w;
    terms8(x, M, Tf, s, w);
    for (int off = 32; off > 0; off >>= 1) {    // (a + b is b + a: every lane ends with the same bits)
        s += __shfl_xor(s, off, 64);
        w += __shfl_xor(w, off, 64);
    }
    if (lane != 0) return;
    const int t = targets[at];
    const bool valid = (unsigned)t < (unsigned)NCLS;
    const float xt = valid ? row[t] : 0.0f;
    finish(at, valid, t, xt, M, s, w, arg, T, nll, entropy, hit);
}

__global__ __launch_bounds__(THREADS) void k_nll_frames(const float *__restrict__ nll, const float *__restrict__ entropy,
                                                        const uint8_t *__restrict__ hit, const uint8_t *__restrict__ region, int L,
                                                        double *__restrict__ frames)
{
    __shared__ double sh[THREADS][8];
    const int t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * L;
    double acc[2][4] = {};
    for (int i = t; i < L; i += THREADS) {
        const int g = region != nullptr && region[base + i] != 0;
        const double v[4] = {1.0, (double)nll[base + i], (double)entropy[base + i], (double)hit[base + i]};
#pragma unroll
        for (int k = 0; k < 4; ++k) {           // (selected, not indexed by g: acc stays in registers)
            acc[0][k] += g ? 0.0 : v[k];
            acc[1][k] += g ? v[k] : 0.0;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) sh[t][k] = acc[k >> 2][k & 3];
    __syncthreads();
    for (int off = THREADS / 2; off > 0; off >>= 1) {
        if (t < off)
#pragma unroll
            for (int k = 0; k < 8; ++k) sh[t][k] += sh[t + off][k];
        __syncthreads();
    }
    if (t < 8) frames[(size_t)blockIdx.x * 8 + t] = sh[0][t];
}

}  // namespace

extern "C" {

const char *ps_nll_last_error(void) { return ps::last_error_ref().c_str(); }

int ps_code_nll_f32(const float *logits, int layout, const int32_t *targets, const uint8_t *region, double temperature, int F, int L,
                    float *nll, float *entropy, uint8_t *hit, double *frames, void *stream)
{
    PS_REQUIRE(logits && targets, "code_nll: null pointer");
    PS_REQUIRE(layout == PS_NLL_LAYOUT_CHW || layout == PS_NLL_LAYOUT_LC, "code_nll: layout = %d, expected 0 (F,512,L) or 1 (F,L,512)", layout);
    PS_REQUIRE(temperature > 0.0 && std::isfinite(temperature), "code_nll: temperature = %g, expected a finite value > 0", temperature);
    PS_REQUIRE(F >= 1 && F <= PS_NLL_MAX_FRAMES, "code_nll: F = %d, expected 1 .. %d", F, PS_NLL_MAX_FRAMES);
    PS_REQUIRE(L >= 1, "code_nll: L = %d, expected >= 1", L);
    PS_REQUIRE(nll || entropy || hit, "code_nll: no output (nll, entropy and hit are all NULL)");
    PS_REQUIRE(!frames || (nll && entropy && hit), "code_nll: frames sums the three per-location outputs: nll, entropy and hit must be given");
    PS_REQUIRE(layout != PS_NLL_LAYOUT_LC || (uintptr_t)logits % 16 == 0, "code_nll: layout 1 needs logits aligned to 16 bytes");
    if (layout == PS_NLL_LAYOUT_CHW)
        hipLaunchKernelGGL(k_code_nll_chw, dim3((L + CHW_LOCS - 1) / CHW_LOCS, F), dim3(THREADS), 0, (hipStream_t)stream, logits, targets,
                           temperature, L, nll, entropy, hit);
    else
        hipLaunchKernelGGL(k_code_nll_lc, dim3((L + LC_LOCS - 1) / LC_LOCS, F), dim3(THREADS), 0, (hipStream_t)stream, logits, targets,
                           temperature, L, nll, entropy, hit);
    PS_LAUNCH_CHECK();
    if (frames) {
        hipLaunchKernelGGL(k_nll_frames, dim3(F), dim3(THREADS), 0, (hipStream_t)stream, nll, entropy, hit, region, L, frames);
        PS_LAUNCH_CHECK();
    }
    return PS_OK;
}

}  // extern "C"
