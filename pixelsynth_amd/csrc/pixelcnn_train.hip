// pixelcnn_train.hip -- what runs between the masked convolutions when the PixelCNN trains, for gfx950 (MI355X): positional
// normalisation + skip + activation (k_norm_act_*), the gate of a gated block (k_gate_*), each forward and backward, and the backward
// pass of the cross entropy of given codes (k_nll_bwd_*).  Behind the C ABI of include/pixelsynth_pixelcnn_train.h
// (libpixelsynth_pixelcnn_train.so); the header states every formula and where it rounds.  Nothing is shared with the engine's post
// ops (lmconv_device.h): those use a fast exponential and a hardware reciprocal, right for sampling and wrong for a gradient; here the
// transcendentals are expf / expm1f and every quotient is a true division.
//
// Lanes run along the LOCATIONS (neighbouring lanes read neighbouring addresses of an NCHW tensor) and walk the channels, which lie L
// values apart.  A location's sums over its channels are four fp64 chains (chain k: channels k, k + 4, ... ascending) joined as
// (s0 + s1) + (s2 + s3).  LPL = lanes per location:
//   LPL = 1   256 locations per workgroup, a lane walks all four chains;
//   LPL = 4   64 locations per workgroup, wavefront k walks chain k of each and the four meet in LDS -- four times the workgroups,
//             for launches that would otherwise leave the compute units short of wavefronts to hide a load behind (16 frames of
//             32 x 32: 64 workgroups for 256 CUs with a lane per location, 256 with four; 64 frames: 256 and 1024).
// The chains are the same sequences of additions in both, so the bits are.  Both forms stream: a pass walks its operands twice (once
// for the sums, once for the results; the second walk hits the cache) and nothing depends on C fitting in registers.
// A lane past the last location works on the last one and writes nothing: every lane reaches every barrier.
#include "ps_common.h"

#include <cmath>

#include "../../include/pixelsynth_pixelcnn_train.h"

namespace {

constexpr int THREADS = 256;
constexpr int NCLS = 512;

template <int LPL> struct Place {
    int p, chain, lane;   // location (clamped), the chain this lane walks (LPL = 4), the location's slot in the workgroup
    bool live;            // whether this lane writes
    __device__ Place(int N)
    {
        lane = LPL == 1 ? (int)threadIdx.x : (int)(threadIdx.x & 63);
        chain = LPL == 1 ? 0 : (int)(threadIdx.x >> 6);
        const long long q = (long long)blockIdx.x * (THREADS / LPL) + lane;
        live = q < N;
        p = live ? (int)q : N - 1;
    }
};

// f(c, k) for the channels c of this lane, k = c & 3 a constant after unrolling: all of them in ascending order (LPL = 1), or those of
// the lane's chain
template <int LPL, typename Fn> __device__ __forceinline__ void walk(int C, int chain, Fn f)
{
#pragma unroll 4
    for (int c0 = 0; c0 < C; c0 += 4) {      // (unrolled: the loads of four rounds are in flight before the first dependent addition)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (c0 + k >= C || (LPL == 4 && k != chain)) continue;
            f(c0 + k, k);
        }
    }
}

// (a0 + a1) + (a2 + a3) of the four chains of a location; with LPL = 4 lane `chain` holds a[chain] and the others' are in other waves
template <int LPL> __device__ __forceinline__ double join(const double (&a)[4], int chain, int lane, double (*sh)[64])
{
    if (LPL == 1) return (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();    // (sh may still be read by the join before)
    sh[chain][lane] = chain == 0 ? a[0] : chain == 1 ? a[1] : chain == 2 ? a[2] : a[3];
    __syncthreads();
    return (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}

__device__ __forceinline__ float elu(float z) { return z > 0.0f ? z : expm1f(z); }
__device__ __forceinline__ float elu_slope(float z) { return z > 0.0f ? 1.0f : expf(z); }
__device__ __forceinline__ float sigmoid(float g) { return 1.0f / (1.0f + expf(-g)); }

// PONO's statistics of the C values at v, v + L, ...: mean and 1 / sqrt(var + eps), each rounded once from fp64
template <int LPL> __device__ __forceinline__ void pono_stats(const float *__restrict__ v, int C, int L, const Place<LPL> &at, double (*sh)[64],
                                                              float &mu, float &rs)
{
    const double K = (double)v[0];
    double s1[4] = {}, s2[4] = {};
    walk<LPL>(C, at.chain, [&](int c, int k) {
        const double d = (double)v[(size_t)c * L] - K;
        s1[k] += d;
        s2[k] += d * d;
    });
    const double S1 = join<LPL>(s1, at.chain, at.lane, sh), S2 = join<LPL>(s2, at.chain, at.lane, sh);
    const double var = (S2 - S1 * S1 / (double)C) / (double)(C - 1);
    mu = (float)(K + S1 / (double)C);
    rs = (float)(1.0 / sqrt((var < 0.0 ? 0.0 : var) + PS_PCT_EPS));
}

__device__ __forceinline__ size_t skip_at(int layout, int b, int l, int p, int c, int C, int L)
{
    return layout == PS_PCT_NHWC ? (size_t)p * C + c : ((size_t)b * C + c) * L + l;
}

template <int LPL>
__global__ __launch_bounds__(THREADS) void k_norm_act_fwd(const float *__restrict__ x, const float *__restrict__ skip, int skip_layout, int N,
                                                          int C, int L, int norm, int act, float *__restrict__ y, float *__restrict__ mean,
                                                          float *__restrict__ rstd)
{
    __shared__ double sh[4][64];
    const Place<LPL> at(N);
    const int b = at.p / L, l = at.p % L;
    const float *xp = x + (size_t)b * C * L + l;
    float mu = 0.0f, rs = 1.0f;
    if (norm) {
        pono_stats<LPL>(xp, C, L, at, sh, mu, rs);
        if (at.live && at.chain == 0) {
            mean[at.p] = mu;
            rstd[at.p] = rs;
        }
    }
    if (!at.live) return;       // (no barrier below)
    const int Cy = act == PS_PCT_ACT_CELU ? 2 * C : C;
    float *yp = y + (size_t)b * Cy * L + l;
    walk<LPL>(C, at.chain, [&](int c, int) {
        const float xv = xp[(size_t)c * L];
        float z = norm ? (xv - mu) * rs : xv;
        if (skip) z = z + skip[skip_at(skip_layout, b, l, at.p, c, C, L)];
        if (act == PS_PCT_ACT_NONE) {
            yp[(size_t)c * L] = z;
        } else {
            yp[(size_t)c * L] = elu(z);
            if (act == PS_PCT_ACT_CELU) yp[(size_t)(C + c) * L] = elu(-z);
        }
    });
}

template <int LPL>
__global__ __launch_bounds__(THREADS) void k_norm_act_bwd(const float *__restrict__ x, const float *__restrict__ skip, int skip_layout,
                                                          const float *__restrict__ dy, const float *__restrict__ mean,
                                                          const float *__restrict__ rstd, int N, int C, int L, int norm, int act,
                                                          float *__restrict__ dx, float *__restrict__ dskip)
{
    __shared__ double sh[4][64];
    const Place<LPL> at(N);
    const int b = at.p / L, l = at.p % L;
    const float *xp = x + (size_t)b * C * L + l;
    const int Cy = act == PS_PCT_ACT_CELU ? 2 * C : C;
    const float *gp = dy + (size_t)b * Cy * L + l;
    const float mu = norm ? mean[at.p] : 0.0f, rs = norm ? rstd[at.p] : 1.0f;
    // channel c -> (dz, xh), as the forward computes z
    auto adjoint = [&](int c, float &xh) {
        const float xv = xp[(size_t)c * L];
        xh = norm ? (xv - mu) * rs : xv;
        float z = xh;
        if (skip) z = z + skip[skip_at(skip_layout, b, l, at.p, c, C, L)];
        const float g1 = gp[(size_t)c * L];
        if (act == PS_PCT_ACT_NONE) return g1;
        if (act == PS_PCT_ACT_ELU) return g1 * elu_slope(z);
        const float lo = g1 * elu_slope(z), hi = gp[(size_t)(C + c) * L] * elu_slope(-z);
        return lo - hi;
    };
    float m1 = 0.0f, m2 = 0.0f;
    if (norm && dx) {
        double a1[4] = {}, a2[4] = {};
        walk<LPL>(C, at.chain, [&](int c, int k) {
            float xh;
            const float dz = adjoint(c, xh);
            a1[k] += (double)dz;
            a2[k] += (double)dz * (double)xh;
        });
        m1 = (float)(join<LPL>(a1, at.chain, at.lane, sh) / (double)C);
        m2 = (float)(join<LPL>(a2, at.chain, at.lane, sh) / (double)(C - 1));
    }
    if (!at.live) return;
    walk<LPL>(C, at.chain, [&](int c, int) {
        float xh;
        const float dz = adjoint(c, xh);
        if (dskip) dskip[skip_at(skip_layout, b, l, at.p, c, C, L)] = dz;
        if (dx) dx[((size_t)b * C + c) * L + l] = norm ? rs * ((dz - m1) - xh * m2) : dz;
    });
}

template <int LPL>
__global__ __launch_bounds__(THREADS) void k_gate_fwd(const float *__restrict__ vg, const float *__restrict__ u, int N, int C, int L,
                                                      float *__restrict__ out, float *__restrict__ mean, float *__restrict__ rstd)
{
    __shared__ double sh[4][64];
    const Place<LPL> at(N);
    const int b = at.p / L, l = at.p % L;
    const float *vp = vg + (size_t)b * 2 * C * L + l, *gp = vp + (size_t)C * L;
    float mu, rs;
    pono_stats<LPL>(vp, C, L, at, sh, mu, rs);
    if (!at.live) return;
    if (at.chain == 0) {
        mean[at.p] = mu;
        rstd[at.p] = rs;
    }
    const size_t base = (size_t)b * C * L + l;
    walk<LPL>(C, at.chain, [&](int c, int) {
        const float vh = (vp[(size_t)c * L] - mu) * rs;
        const float gated = vh * sigmoid(gp[(size_t)c * L]);
        out[base + (size_t)c * L] = u[base + (size_t)c * L] + gated;
    });
}

template <int LPL>
__global__ __launch_bounds__(THREADS) void k_gate_bwd(const float *__restrict__ vg, const float *__restrict__ dout, const float *__restrict__ mean,
                                                      const float *__restrict__ rstd, int N, int C, int L, float *__restrict__ dvg)
{
    __shared__ double sh[4][64];
    const Place<LPL> at(N);
    const int b = at.p / L, l = at.p % L;
    const float *vp = vg + (size_t)b * 2 * C * L + l, *gp = vp + (size_t)C * L;
    const float *dp = dout + (size_t)b * C * L + l;
    const float mu = mean[at.p], rs = rstd[at.p];
    double a1[4] = {}, a2[4] = {};
    walk<LPL>(C, at.chain, [&](int c, int k) {
        const float vh = (vp[(size_t)c * L] - mu) * rs;
        const float a = dp[(size_t)c * L] * sigmoid(gp[(size_t)c * L]);
        a1[k] += (double)a;
        a2[k] += (double)a * (double)vh;
    });
    const float m1 = (float)(join<LPL>(a1, at.chain, at.lane, sh) / (double)C);
    const float m2 = (float)(join<LPL>(a2, at.chain, at.lane, sh) / (double)(C - 1));
    if (!at.live) return;
    float *dvp = dvg + (size_t)b * 2 * C * L + l, *dgp = dvp + (size_t)C * L;
    walk<LPL>(C, at.chain, [&](int c, int) {
        const float vh = (vp[(size_t)c * L] - mu) * rs;
        const float d = dp[(size_t)c * L], s = sigmoid(gp[(size_t)c * L]);
        const float a = d * s;
        dvp[(size_t)c * L] = rs * ((a - m1) - vh * m2);
        const float ds = s * (1.0f - s);
        dgp[(size_t)c * L] = (d * vh) * ds;
    });
}

// ---------------------------------------------------------------------------------------------------- the cross entropy's backward
// fp32(double(grad_out) / count / T), count = the chosen groups' counts over the frames (integers held in fp64: exact in any order).
// Once per WAVEFRONT, all 64 lanes together: lane l adds the frames l, l + 64, ..., a butterfly adds the lanes -- ceil(F / 64) rounds of
// loads per wavefront, not F per lane
__device__ __forceinline__ float nll_scale(const double *__restrict__ frames, int groups, int F, double T, const float *__restrict__ grad_out,
                                           int lane)
{
    double count = 0.0;
    for (int f = lane; f < F; f += 64) {
        if (groups & PS_PCT_GROUP_OBSERVED) count += frames[(size_t)f * 8];
        if (groups & PS_PCT_GROUP_SAMPLED) count += frames[(size_t)f * 8 + 4];
    }
    for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off, 64);
    return (float)((double)grad_out[0] / count / T);
}

__device__ __forceinline__ bool in_groups(const uint8_t *__restrict__ region, size_t at, int groups)
{
    const int g = region != nullptr && region[at] != 0;
    return (groups >> g) & 1;
}

constexpr int CHW_LOCS = 64, CHW_CLS = NCLS / 4;

// (F,512,L): a workgroup per 64 consecutive locations, lanes across the locations, wave w holds classes 128 w .. 128 w + 127
__global__ __launch_bounds__(THREADS) void k_nll_bwd_chw(const float *__restrict__ logits, const int32_t *__restrict__ targets,
                                                         const uint8_t *__restrict__ region, const double *__restrict__ frames, int groups,
                                                         double T, int F, int L, const float *__restrict__ grad_out, float *__restrict__ grad)
{
    __shared__ float sh[4][CHW_LOCS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.y;
    const int loc = blockIdx.x * CHW_LOCS + lane;
    const bool live = loc < L;
    const int q = live ? loc : L - 1;
    const size_t at = (size_t)f * L + q;
    const bool in = in_groups(region, at, groups);     // (the same in the four waves of a location)
    const int c0 = wave * CHW_CLS;
    const size_t base = ((size_t)f * NCLS + c0) * (size_t)L + q;
    float x[CHW_CLS];
    if (in) {
#pragma unroll
        for (int k = 0; k < CHW_CLS; ++k) x[k] = logits[base + (size_t)k * L];
    } else {
#pragma unroll
        for (int k = 0; k < CHW_CLS; ++k) x[k] = 0.0f;
    }
    float best = -INFINITY;
#pragma unroll
    for (int k = 0; k < CHW_CLS; ++k) best = x[k] > best ? x[k] : best;      // (a NaN is never larger)
    sh[wave][lane] = best;
    __syncthreads();
    float M = sh[0][lane];
#pragma unroll
    for (int v = 1; v < 4; ++v) M = sh[v][lane] > M ? sh[v][lane] : M;
    __syncthreads();
    const float Tf = (float)T;
    float part[8] = {};
#pragma unroll
    for (int k = 0; k < CHW_CLS; ++k) {
        x[k] = expf((x[k] - M) / Tf);
        part[k & 7] += x[k];
    }
    sh[wave][lane] = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
    __syncthreads();
    const float scale = nll_scale(frames, groups, F, T, grad_out, lane);      // (every lane of the wavefront: before the dead ones leave)
    if (!live) return;
    const float s = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
    const int t = targets[at];
    const bool bad = (unsigned)t >= (unsigned)NCLS || s != s;
#pragma unroll
    for (int k = 0; k < CHW_CLS; ++k) {
        const float d = x[k] / s - (c0 + k == t ? 1.0f : 0.0f);
        grad[base + (size_t)k * L] = !in ? 0.0f : bad ? NAN : scale * d;
    }
}

// (F,L,512): a wave per location, lane l holds classes 8 l .. 8 l + 7
__global__ __launch_bounds__(THREADS) void k_nll_bwd_lc(const float *__restrict__ logits, const int32_t *__restrict__ targets,
                                                        const uint8_t *__restrict__ region, const double *__restrict__ frames, int groups,
                                                        double T, int F, int L, const float *__restrict__ grad_out, float *__restrict__ grad)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.y;
    const int loc = blockIdx.x * 4 + wave;
    if (loc >= L) return;                       // (whole waves; the kernel has no barrier)
    const size_t at = (size_t)f * L + loc;
    float4 *out = reinterpret_cast<float4 *>(grad + at * NCLS) + lane * 2;
    if (!in_groups(region, at, groups)) {
        out[0] = out[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 *row = reinterpret_cast<const float4 *>(logits + at * NCLS) + lane * 2;
    const float4 lo = row[0], hi = row[1];
    float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    float M = -INFINITY;
#pragma unroll
    for (int k = 0; k < 8; ++k) M = x[k] > M ? x[k] : M;
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(M, off, 64);
        M = o > M ? o : M;
    }
    const float Tf = (float)T;
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = expf((x[k] - M) / Tf);
    float s = ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]));
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);      // (a + b is b + a: every lane ends with the same bits)
    const int t = targets[at];
    const bool bad = (unsigned)t >= (unsigned)NCLS || s != s;
    const float scale = nll_scale(frames, groups, F, T, grad_out, lane);      // (the wavefront is whole here: a location is one)
    float r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float d = x[k] / s - (lane * 8 + k == t ? 1.0f : 0.0f);
        r[k] = bad ? NAN : scale * d;
    }
    out[0] = make_float4(r[0], r[1], r[2], r[3]);
    out[1] = make_float4(r[4], r[5], r[6], r[7]);
}

int check_sizes(const char *who, int B, int C, int L, int min_c)
{
    PS_REQUIRE(B >= 1 && L >= 1, "%s: B = %d, L = %d, expected >= 1", who, B, L);
    PS_REQUIRE((long long)B * L < (1ll << 31), "%s: B * L = %lld locations, expected fewer than 2^31", who, (long long)B * L);
    PS_REQUIRE(C >= min_c && C <= PS_PCT_MAX_CHANNELS, "%s: C = %d, expected %d .. %d", who, C, min_c, PS_PCT_MAX_CHANNELS);
    return PS_OK;
}

// KERNEL<4> or KERNEL<1> over N locations, by ps_pixelcnn_train_lanes
#define PS_PCT_LAUNCH(KERNEL, N, stream, ...)                                                                                        \
    do {                                                                                                                             \
        if (ps_pixelcnn_train_lanes(N) == 4)                                                                                         \
            hipLaunchKernelGGL(KERNEL<4>, dim3((unsigned)(((N) + 63) / 64)), dim3(THREADS), 0, (hipStream_t)(stream), __VA_ARGS__);  \
        else                                                                                                                         \
            hipLaunchKernelGGL(KERNEL<1>, dim3((unsigned)(((N) + 255) / 256)), dim3(THREADS), 0, (hipStream_t)(stream), __VA_ARGS__); \
        PS_LAUNCH_CHECK();                                                                                                           \
    } while (0)

}  // namespace

extern "C" {

const char *ps_pixelcnn_train_last_error(void) { return ps::last_error_ref().c_str(); }

int ps_pixelcnn_train_lanes(long long N) { return N < 1 ? 0 : N < PS_PCT_WIDE_LOCATIONS ? 4 : 1; }

int ps_norm_act_forward_f32(const float *x, const float *skip, int skip_layout, int B, int C, int L, int norm, int act, float *y,
                            float *mean, float *rstd, void *stream)
{
    PS_REQUIRE(x && y, "norm_act forward: null pointer");
    PS_REQUIRE(!norm || (mean && rstd), "norm_act forward: with norm set, mean and rstd are outputs");
    PS_REQUIRE(act >= PS_PCT_ACT_NONE && act <= PS_PCT_ACT_CELU, "norm_act forward: act = %d, expected 0 .. 2", act);
    PS_REQUIRE(skip_layout == PS_PCT_NCHW || skip_layout == PS_PCT_NHWC, "norm_act forward: skip_layout = %d, expected 0 or 1", skip_layout);
    if (int rc = check_sizes("norm_act forward", B, C, L, norm ? 2 : 1)) return rc;
    const int N = B * L;
    PS_PCT_LAUNCH(k_norm_act_fwd, N, stream, x, skip, skip_layout, N, C, L, norm, act, y, mean, rstd);
    return PS_OK;
}

int ps_norm_act_backward_f32(const float *x, const float *skip, int skip_layout, const float *dy, const float *mean, const float *rstd,
                             int B, int C, int L, int norm, int act, float *dx, float *dskip, void *stream)
{
    PS_REQUIRE(x && dy, "norm_act backward: null pointer");
    PS_REQUIRE(dx || dskip, "norm_act backward: no output (dx and dskip are both NULL)");
    PS_REQUIRE(!norm || (mean && rstd), "norm_act backward: with norm set, mean and rstd are inputs");
    PS_REQUIRE(act >= PS_PCT_ACT_NONE && act <= PS_PCT_ACT_CELU, "norm_act backward: act = %d, expected 0 .. 2", act);
    PS_REQUIRE(skip_layout == PS_PCT_NCHW || skip_layout == PS_PCT_NHWC, "norm_act backward: skip_layout = %d, expected 0 or 1", skip_layout);
    if (int rc = check_sizes("norm_act backward", B, C, L, norm ? 2 : 1)) return rc;
    const int N = B * L;
    PS_PCT_LAUNCH(k_norm_act_bwd, N, stream, x, skip, skip_layout, dy, mean, rstd, N, C, L, norm, act, dx, dskip);
    return PS_OK;
}

int ps_gate_forward_f32(const float *vg, const float *u, int B, int C, int L, float *out, float *mean, float *rstd, void *stream)
{
    PS_REQUIRE(vg && u && out && mean && rstd, "gate forward: null pointer");
    if (int rc = check_sizes("gate forward", B, C, L, 2)) return rc;
    const int N = B * L;
    PS_PCT_LAUNCH(k_gate_fwd, N, stream, vg, u, N, C, L, out, mean, rstd);
    return PS_OK;
}

int ps_gate_backward_f32(const float *vg, const float *dout, const float *mean, const float *rstd, int B, int C, int L, float *dvg,
                         void *stream)
{
    PS_REQUIRE(vg && dout && mean && rstd && dvg, "gate backward: null pointer");
    if (int rc = check_sizes("gate backward", B, C, L, 2)) return rc;
    const int N = B * L;
    PS_PCT_LAUNCH(k_gate_bwd, N, stream, vg, dout, mean, rstd, N, C, L, dvg);
    return PS_OK;
}

int ps_code_nll_backward_f32(const float *logits, int layout, const int32_t *targets, const uint8_t *region, const double *frames,
                             int groups, double temperature, int F, int L, const float *grad_out, float *grad_logits, void *stream)
{
    PS_REQUIRE(logits && targets && frames && grad_out && grad_logits, "code_nll backward: null pointer");
    PS_REQUIRE(layout == 0 || layout == 1, "code_nll backward: layout = %d, expected 0 (F,512,L) or 1 (F,L,512)", layout);
    PS_REQUIRE(groups >= 1 && groups <= 3, "code_nll backward: groups = %d, expected 1 (observed), 2 (sampled) or 3 (all)", groups);
    PS_REQUIRE(temperature > 0.0 && std::isfinite(temperature), "code_nll backward: temperature = %g, expected a finite value > 0", temperature);
    PS_REQUIRE(F >= 1 && F <= 65535, "code_nll backward: F = %d, expected 1 .. 65535", F);
    PS_REQUIRE(L >= 1, "code_nll backward: L = %d, expected >= 1", L);
    PS_REQUIRE(layout != 1 || (ps::aligned16(logits) && ps::aligned16(grad_logits)), "code_nll backward: layout 1 needs logits and their gradient aligned to 16 bytes");
    if (layout == 0)
        hipLaunchKernelGGL(k_nll_bwd_chw, dim3((L + CHW_LOCS - 1) / CHW_LOCS, F), dim3(THREADS), 0, (hipStream_t)stream, logits, targets,
                           region, frames, groups, temperature, F, L, grad_out, grad_logits);
    else
        hipLaunchKernelGGL(k_nll_bwd_lc, dim3((L + 3) / 4, F), dim3(THREADS), 0, (hipStream_t)stream, logits, targets, region, frames,
                           groups, temperature, F, L, grad_out, grad_logits);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
