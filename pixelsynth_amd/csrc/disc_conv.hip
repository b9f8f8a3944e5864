// disc_conv.hip -- the discriminator's 4 x 4 convolution (stride 1 or 2, padding 2, no bias) with its backward pass for gfx950 (MI355X),
// on the fp16 matrix pipe with split operands, for dense NCHW fp32 tensors.  Behind the C ABI of include/pixelsynth_disc_conv.h
// (libpixelsynth_disc_conv.so), which states the arithmetic, the sum orders, the plan's formulas and the overflow rules.
//
// The weight IS scaled: weight_orig / sigma has entries around 1e-2, where the lo half of the split is a subnormal fp16 and the pair keeps
// some 17 bits; times a power of two that brings max|w| into [2^14, 2^15) it keeps its 22.  grad_y gets the same treatment
// (csrc/conv_bwd.hip's rule); x is split as it is.
//
// Layouts are converted in passes of their own, so that the products read every operand with aligned 16-byte loads and need no LDS:
//   k_disc_conv_amax_partial / _finish   max|v| of a tensor -> {s, 1 / s} on the device
//   k_disc_conv_pack                     w * sw -> [tap][out channel][in channel] fp16 hi / lo (three tap orders: forward, grad_x stride 1 / 2)
//   k_disc_conv_nhwc                     NCHW fp32 (times s) -> channels-last split fp16 with the zero border written out (an LDS transpose)
//   k_disc_conv_rows                     NCHW fp32 (times s) -> pixel-minor split fp16 in rows of Wo8, one plane per kx, for grad_weight
//   k_disc_conv_mfma                     the implicit GEMM of y and of grad_x: a wave owns 64 output channels x 64 output pixels of one frame
//                                        (four 32 x 32 accumulators); A = weight [m = out channel][k = in channel], B = input
//                                        [k = in channel][n = pixel], one tap and 16 channels per MFMA step; D's columns are pixels,
//                                        so a store is 32 consecutive floats of an NCHW row
//   k_disc_conv_gw_parts                 grad_weight: a wave owns 64 output channels x 32 input channels x the four kx of one ky (eight
//                                        accumulators); A = g [m = out channel][k = pixel], B = x [k = pixel][n = in channel], 16
//                                        pixels per step; the four waves of a workgroup are the four ky
//   k_disc_conv_gw_sum                   adds the parts in ascending order, times 1 / sg, into (Co,Ci,4,4)
// No atomics, vector stores only.
#include "ps_common.h"

#include <cfloat>
#include <cmath>

#include "../../include/pixelsynth_disc_conv.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NT = 256;
constexpr int AMAX_BLOCKS = 256;
constexpr int TARGET_WGS = 512;
constexpr int MIN_CHUNK = 8;
constexpr long long LIM = 1LL << 31;

inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

struct Plan {
    int Ho, Wo, Hp, Wp, Wo8, nch, Q, spf, steps, blocks, chunk, parts;
    size_t o_amax, o_wscale, o_wp, o_xs, o_gn, o_gt, o_xt, o_part, bytes;   // byte offsets into the workspace
    size_t n_wp, n_xs, n_gn, n_gt, n_xt;                                    // halves per plane (hi; lo follows)
};

inline bool sizes_ok(int B, int Ci, int Co, int H, int W, int stride, int pad)
{
    if (!(B >= 1 && B <= 65535 && (stride == 1 || stride == 2) && pad == 2 && H >= 1 && W >= 1 && Ci >= 64 && Co >= 64 && Ci <= 512 && Co <= 512
          && Ci % 64 == 0 && Co % 64 == 0 && H < (1 << 24) && W < (1 << 24)))
        return false;
    const long long Hp = H + 2 * pad, Wp = W + 2 * pad, Ho = (Hp - 4) / stride + 1, Wo = (Wp - 4) / stride + 1, Wo8 = cdiv(Wo, 8) * 8;
    return Hp * Wp * Ci < LIM && (Ho + 2) * (Wo + 2) * Co < LIM && Ci * Hp * Wo8 < LIM && Co * Ho * Wo8 < LIM
           && B * cdiv(Ho * (Wo8 / 8), 2) < LIM;
}

inline Plan make_plan(int B, int Ci, int Co, int H, int W, int stride, int pad)
{
    Plan p;
    p.Hp = H + 2 * pad; p.Wp = W + 2 * pad;
    p.Ho = (p.Hp - 4) / stride + 1; p.Wo = (p.Wp - 4) / stride + 1;
    p.Wo8 = (p.Wo + 7) / 8 * 8; p.nch = p.Wo8 / 8;
    p.Q = p.Ho * p.nch; p.spf = (p.Q + 1) / 2; p.steps = B * p.spf;
    p.blocks = (Co / 64) * (Ci / 32);
    long long want = cdiv(TARGET_WGS, p.blocks);
    if (want > PS_DISC_CONV_MAX_PARTS) want = PS_DISC_CONV_MAX_PARTS;
    p.chunk = (int)cdiv(p.steps, want);
    if (p.chunk < MIN_CHUNK) p.chunk = MIN_CHUNK;
    p.parts = (int)cdiv(p.steps, p.chunk);
    p.n_wp = (size_t)16 * Co * Ci;
    p.n_xs = (size_t)B * p.Hp * p.Wp * Ci;
    p.n_gn = (size_t)B * (p.Ho + 2) * (p.Wo + 2) * Co;
    p.n_gt = (size_t)B * Co * p.Ho * p.Wo8;
    p.n_xt = (size_t)4 * B * Ci * p.Hp * p.Wo8;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = ps::align_up(o + bytes, 256); return at; };
    p.o_amax = take(AMAX_BLOCKS * sizeof(float));
    p.o_wscale = take(2 * sizeof(float));
    p.o_wp = take(p.n_wp * 4);
    p.o_xs = take(p.n_xs * 4);
    p.o_gn = take(p.n_gn * 4);
    p.o_gt = take(p.n_gt * 4);
    p.o_xt = take(p.n_xt * 4);
    p.o_part = take((size_t)p.parts * 16 * Co * Ci * sizeof(float));
    p.bytes = o;
    return p;
}

// ---- max|v| -> {s, 1 / s} ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_disc_conv_amax_partial(const float *__restrict__ v, size_t n, float *__restrict__ part)
{
    __shared__ float sh[NT];
    float m = 0.0f;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
        const float a = __builtin_fabsf(v[i]);
        bad |= !(a <= FLT_MAX);
        m = a > m ? a : m;
    }
    sh[threadIdx.x] = bad ? INFINITY : m;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] = sh[threadIdx.x] > sh[threadIdx.x + off] ? sh[threadIdx.x] : sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// s = 2^(15 - e), max = f * 2^e with f in [0.5, 1); the exponent held in [-126, 126]; 1 for a maximum of 0 or one that is not finite
__global__ __launch_bounds__(NT) void k_disc_conv_amax_finish(const float *__restrict__ part, int n, float *__restrict__ scale2)
{
    __shared__ float sh[NT];
    float m = 0.0f;
    for (int i = threadIdx.x; i < n; i += NT) m = part[i] > m ? part[i] : m;
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] = sh[threadIdx.x] > sh[threadIdx.x + off] ? sh[threadIdx.x] : sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        m = sh[0];
        float s = 1.0f, inv = 1.0f;
        if (m > 0.0f && m <= FLT_MAX) {
            int e;
            (void)frexpf(m, &e);
            int k = 15 - e;
            k = k > 126 ? 126 : k < -126 ? -126 : k;
            s = ldexpf(1.0f, k);
            inv = ldexpf(1.0f, -k);
        }
        scale2[0] = s;
        scale2[1] = inv;
    }
}

__device__ __forceinline__ void split1(float v, _Float16 &hi, _Float16 &lo)
{
    hi = (_Float16)v;
    lo = (_Float16)(v - (float)hi);
}

// ---- the weight: (Co,Ci,4,4) fp32 -> [16 taps][out][in] fp16 hi / lo of w * sw.  mode 0: forward (out = o, in = c); 1: grad_x at stride 1;
// 2: grad_x at stride 2 (out = c, in = o).  A thread owns one (o, c) pair and its 16 taps; consecutive threads are consecutive `in`.
__global__ __launch_bounds__(NT) void k_disc_conv_pack(const float *__restrict__ w, const float *__restrict__ wscale2, int mode, int Co, int Ci,
                                                       _Float16 *__restrict__ hi, _Float16 *__restrict__ lo, int *overflow)
{
    const int idx = blockIdx.x * NT + threadIdx.x;
    if (idx >= Co * Ci) return;
    const int n_out = mode == 0 ? Co : Ci, n_in = mode == 0 ? Ci : Co;
    const int vo = idx / n_in, vi = idx - vo * n_in;
    const int o = mode == 0 ? vo : vi, c = mode == 0 ? vi : vo;
    const float s = wscale2[0];
    const float *src = w + ((size_t)o * Ci + c) * 16;
    int over = 0;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int ky = t >> 2, kx = t & 3;
        const int u = mode == 0 ? t : mode == 1 ? 4 * (3 - ky) + (3 - kx) : 4 * (2 * (ky & 1) + (kx & 1)) + 2 * (1 - (ky >> 1)) + (1 - (kx >> 1));
        const float v = src[t] * s;
        over |= !(__builtin_fabsf(v) <= 65000.f);
        _Float16 h, l;
        split1(v, h, l);
        const size_t at = ((size_t)u * n_out + vo) * n_in + vi;
        hi[at] = h;
        lo[at] = l;
    }
    if (over) *overflow = 1;
}

// ---- NCHW fp32 (B,C,H,W) times s -> channels-last split fp16 (B,H + 2P,W + 2P,C) with the zero border.  grid (ceil(Hp Wp / 32), C / 64, B):
// a workgroup transposes 32 padded pixels x 64 channels through LDS.
__global__ __launch_bounds__(NT) void k_disc_conv_nhwc(const float *__restrict__ in, const float *__restrict__ scale2, int C, int H, int W, int P,
                                                       _Float16 *__restrict__ hi, _Float16 *__restrict__ lo, int *overflow)
{
    __shared__ float tile[64][33];
    const int t = threadIdx.x, Hp = H + 2 * P, Wp = W + 2 * P, NPp = Hp * Wp;
    const int c0 = blockIdx.y * 64, b = blockIdx.z, pp0 = blockIdx.x * 32;
    const float s = scale2 ? scale2[0] : 1.0f;
    {
        const int px = t & 31, cc = t >> 5, pp = pp0 + px;
        const int yp = pp / Wp, xp = pp - yp * Wp, y = yp - P, x = xp - P;
        const bool in_frame = pp < NPp && y >= 0 && y < H && x >= 0 && x < W;
        const float *src = in + ((size_t)b * C + c0 + cc) * H * W + (in_frame ? y * W + x : 0);
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[cc + 8 * i][px] = in_frame ? src[(size_t)8 * i * H * W] * s : 0.0f;
    }
    __syncthreads();
    const int c = t & 63, pr = t >> 6;
    int over = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int px = pr + 4 * i, pp = pp0 + px;
        if (pp >= NPp) continue;
        const float v = tile[c][px];
        over |= !(__builtin_fabsf(v) <= 65000.f);
        _Float16 h, l;
        split1(v, h, l);
        const size_t at = ((size_t)b * NPp + pp) * C + c0 + c;
        hi[at] = h;
        lo[at] = l;
    }
    if (over) *overflow = 1;
}

// ---- NCHW fp32 (planes,H,W) times s -> pixel-minor split fp16 (nkx, planes, R, Wo8):  out[kx][plane][r][j] = in[plane][r - P][j st + kx - P]
// for j < Wo and an index inside the frame, else 0.  A thread owns one chunk of 8 values of j (one 16-byte store per half).
__global__ __launch_bounds__(NT) void k_disc_conv_rows(const float *__restrict__ in, const float *__restrict__ scale2, size_t planes, int H, int W,
                                                       int R, int P, int st, int nkx, int Wo, int nch, _Float16 *__restrict__ hi,
                                                       _Float16 *__restrict__ lo, int *overflow)
{
    const size_t total = (size_t)nkx * planes * R * nch;
    const float s = scale2 ? scale2[0] : 1.0f;
    int over = 0;
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < total; e += (size_t)gridDim.x * NT) {
        const int ch = (int)(e % nch);
        const size_t row = e / nch;                   // (kx * planes + plane) * R + r
        const int r = (int)(row % R);
        const size_t kp = row / R;
        const int kx = (int)(kp / planes);
        const size_t plane = kp - (size_t)kx * planes;
        const int y = r - P;
        const float *src = in + plane * H * W + (size_t)(y >= 0 && y < H ? y : 0) * W;
        h8 vh, vl;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int jj = ch * 8 + j, x = jj * st + kx - P;
            float v = 0.0f;
            if (jj < Wo && y >= 0 && y < H && x >= 0 && x < W) v = src[x] * s;
            over |= !(__builtin_fabsf(v) <= 65000.f);
            _Float16 h, l;
            split1(v, h, l);
            vh[j] = h;
            vl[j] = l;
        }
        *(h8 *)(hi + e * 8) = vh;
        *(h8 *)(lo + e * 8) = vl;
    }
    if (over) *overflow = 1;
}

inline unsigned stream_grid(size_t n)
{
    const size_t want = (n + NT - 1) / NT;
    return (unsigned)(want < (1u << 16) ? (want ? want : 1) : (1u << 16));
}

// ---- y and grad_x: the implicit GEMM ---------------------------------------------------------------------------------------------------------
struct ConvArgs {
    const _Float16 *in_hi, *in_lo;    // (B, Hp, Wp, Cin), the border written out
    const _Float16 *w_hi, *w_lo;      // [tap][Cout][Cin], from this launch's first tap
    const float *wscale2, *gscale2;   // {s, 1 / s} of the weight; of grad_y, or null
    float *out;                       // (B, Cout, Hout, Wout)
    int Hp, Wp, Cin, Cout, Hout, Wout;
    int Hm, Wm;                       // the output pixels of this launch: (m, n) -> (m os + oy0, n os + ox0)
    int s, off, KH, KW, os, oy0, ox0; // input pixel of tap (ty, tx): (m s + ty + off, n s + tx + off) of the padded frame
};

// grid (ceil(Hm Wm / 256), Cout / 64, B); wave w of a workgroup owns the pixels 64 (4 blockIdx.x + w) .. + 63 of the launch's Hm x Wm
__global__ __launch_bounds__(NT) void k_disc_conv_mfma(ConvArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, kb = lane >> 5;
    const int NP = a.Hm * a.Wm, n0 = ((int)blockIdx.x * 4 + wave) * 64;
    if (n0 >= NP) return;                                  // (no barrier in this kernel)
    const int o0 = blockIdx.y * 64, b = blockIdx.z, Cin = a.Cin, Cout = a.Cout;
    int inoff[2], outoff[2];
    bool valid[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int n = n0 + 32 * nb + col;
        valid[nb] = n < NP;
        const int nc = valid[nb] ? n : NP - 1, m = nc / a.Wm, nn = nc - m * a.Wm;
        inoff[nb] = ((m * a.s + a.off) * a.Wp + nn * a.s + a.off) * Cin + 8 * kb;
        outoff[nb] = (m * a.os + a.oy0) * a.Wout + nn * a.os + a.ox0;
    }
    const _Float16 *ih = a.in_hi + (size_t)b * a.Hp * a.Wp * Cin, *il = a.in_lo + (size_t)b * a.Hp * a.Wp * Cin;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i >> 1][i & 1][r] = 0.f;

    // One step is one tap and 16 input channels: eight 16-byte loads and twelve MFMAs.  The fragments of step i + 1 are fetched before
    // the MFMAs of step i are issued (two sets of registers, the loop unrolled by two), in the same order of sums as a plain loop.
    struct Frag { h8 ah[2], al[2], bh[2], bl[2]; };
    const int steps = a.KH * a.KW * (Cin / 16);          // (even: Cin is a multiple of 64)
    int lu = 0, lc = 0;                                  // the tap and the first channel of the next step to fetch
    auto fetch = [&](Frag &f) {
        const int ty = lu / a.KW, tx = lu - ty * a.KW, tapoff = (ty * a.Wp + tx) * Cin + lc;
        const size_t wat = ((size_t)lu * Cout + o0 + col) * Cin + 8 * kb + lc;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            f.ah[mb] = *(const h8 *)(a.w_hi + wat + (size_t)mb * 32 * Cin);
            f.al[mb] = *(const h8 *)(a.w_lo + wat + (size_t)mb * 32 * Cin);
        }
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            f.bh[nb] = *(const h8 *)(ih + inoff[nb] + tapoff);
            f.bl[nb] = *(const h8 *)(il + inoff[nb] + tapoff);
        }
        lc += 16;
        if (lc == Cin) { lc = 0; ++lu; }
    };
    auto mac = [&](const Frag &f) {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[mb], f.bh[nb], acc[mb][nb], 0, 0, 0);
                acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[mb], f.bl[nb], acc[mb][nb], 0, 0, 0);
                acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[mb], f.bh[nb], acc[mb][nb], 0, 0, 0);
            }
    };
    Frag f0, f1;
    fetch(f0);
    for (int step = 0; step < steps; step += 2) {
        fetch(f1);
        mac(f0);
        if (step + 2 < steps) fetch(f0);
        mac(f1);
    }
    // D[row][col]: col = lane & 31 = pixel, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) = output channel
    const float fw = a.wscale2[1], fg = a.gscale2 ? a.gscale2[1] : 1.0f;
    const size_t plane = (size_t)a.Hout * a.Wout;
    float *ob = a.out + ((size_t)b * Cout + o0) * plane;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        if (!valid[nb]) continue;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * mb + (r & 3) + 8 * (r >> 2) + 4 * kb;
                ob[(size_t)row * plane + outoff[nb]] = (acc[mb][nb][r] * fw) * fg;
            }
    }
}

// ---- grad_weight ---------------------------------------------------------------------------------------------------------------------------
struct GwArgs {
    const _Float16 *g_hi, *g_lo;     // (B, Co, Ho, Wo8) scaled
    const _Float16 *x_hi, *x_lo;     // (4, B, Ci, Hp, Wo8)
    float *part;                     // (parts, 16, Co, Ci)
    int B, Ci, Co, Ho, Hp, Wo8, nch, Q, spf, steps, chunk, s, ncib;
};

// grid (parts, (Co / 64) (Ci / 32)); wave = ky
__global__ __launch_bounds__(NT) void k_disc_conv_gw_parts(GwArgs a)
{
    const int lane = threadIdx.x & 63, ky = threadIdx.x >> 6, col = lane & 31, kb = lane >> 5;
    const int o0 = ((int)blockIdx.y / a.ncib) * 64, c0 = ((int)blockIdx.y % a.ncib) * 32;
    const int st0 = blockIdx.x * a.chunk, st1 = min(st0 + a.chunk, a.steps);
    const size_t gplane = (size_t)a.Ho * a.Wo8, xplane = (size_t)a.Hp * a.Wo8;
    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i >> 2][i & 3][r] = 0.f;

    for (int st = st0; st < st1; ++st) {
        const int b = st / a.spf, i = st - b * a.spf, q = 2 * i + kb;
        const bool valid = q < a.Q;
        const int qc = valid ? q : 0, oy = qc / a.nch, ch = qc - oy * a.nch;
        const size_t gat = ((size_t)b * a.Co + o0 + col) * gplane + (size_t)oy * a.Wo8 + ch * 8;
        const size_t xat = ((size_t)b * a.Ci + c0 + col) * xplane + (size_t)(oy * a.s + ky) * a.Wo8 + ch * 8;
        h8 ah[2], al[2];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            ah[mb] = *(const h8 *)(a.g_hi + gat + (size_t)mb * 32 * gplane);
            al[mb] = *(const h8 *)(a.g_lo + gat + (size_t)mb * 32 * gplane);
            if (!valid) {
#pragma unroll
                for (int j = 0; j < 8; ++j) ah[mb][j] = al[mb][j] = (_Float16)0.0f;
            }
        }
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) {
            const size_t xk = xat + (size_t)kx * a.B * a.Ci * xplane;
            const h8 bh = *(const h8 *)(a.x_hi + xk), bl = *(const h8 *)(a.x_lo + xk);
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                acc[mb][kx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[mb], bh, acc[mb][kx], 0, 0, 0);
                acc[mb][kx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mb], bl, acc[mb][kx], 0, 0, 0);
                acc[mb][kx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mb], bh, acc[mb][kx], 0, 0, 0);
            }
        }
    }
    // D[row][col]: col = lane & 31 = input channel, row = output channel
#pragma unroll
    for (int kx = 0; kx < 4; ++kx) {
        float *out = a.part + (((size_t)blockIdx.x * 16 + 4 * ky + kx) * a.Co + o0) * a.Ci + c0 + col;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * mb + (r & 3) + 8 * (r >> 2) + 4 * kb;
                out[(size_t)row * a.Ci] = acc[mb][kx][r];
            }
    }
}

// grad_W[o,c,t] = (part 0 + part 1 + ...)[t,o,c] / sg, in that order; a thread owns one element, consecutive threads consecutive c
__global__ __launch_bounds__(NT) void k_disc_conv_gw_sum(const float *__restrict__ part, int parts, int Co, int Ci, const float *__restrict__ scale2,
                                                         float *__restrict__ gw)
{
    const size_t n = (size_t)16 * Co * Ci, e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e >= n) return;
    float s = part[e];
    for (int p = 1; p < parts; ++p) s += part[(size_t)p * n + e];
    const int c = (int)(e % Ci), o = (int)((e / Ci) % Co), t = (int)(e / ((size_t)Ci * Co));
    gw[((size_t)o * Ci + c) * 16 + t] = s * scale2[1];
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
int amax_scale(const float *v, size_t n, float *partial, float *scale2, hipStream_t st)
{
    size_t want = (n + (size_t)NT * 8 - 1) / ((size_t)NT * 8);
    const int nblk = (int)(want < 1 ? 1 : want > AMAX_BLOCKS ? AMAX_BLOCKS : want);
    hipLaunchKernelGGL(k_disc_conv_amax_partial, dim3(nblk), dim3(NT), 0, st, v, n, partial);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_disc_conv_amax_finish, dim3(1), dim3(NT), 0, st, (const float *)partial, nblk, scale2);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int pack_weight(const float *w, const float *wscale2, int mode, int Co, int Ci, _Float16 *hi, int *overflow, hipStream_t st)
{
    hipLaunchKernelGGL(k_disc_conv_pack, dim3((Co * Ci + NT - 1) / NT), dim3(NT), 0, st, w, wscale2, mode, Co, Ci, hi, hi + (size_t)16 * Co * Ci,
                       overflow);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int to_nhwc(const float *in, const float *scale2, int B, int C, int H, int W, int P, _Float16 *hi, size_t n, int *overflow, hipStream_t st)
{
    const int NPp = (H + 2 * P) * (W + 2 * P);
    hipLaunchKernelGGL(k_disc_conv_nhwc, dim3((NPp + 31) / 32, C / 64, B), dim3(NT), 0, st, in, scale2, C, H, W, P, hi, hi + n, overflow);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int launch_conv(const ConvArgs &a, int B, hipStream_t st)
{
    if (a.Hm <= 0 || a.Wm <= 0) return PS_OK;
    // the farthest input pixel a tap reads lies inside the padded frame
    PS_REQUIRE((a.Hm - 1) * a.s + a.KH - 1 + a.off < a.Hp && (a.Wm - 1) * a.s + a.KW - 1 + a.off < a.Wp
               && (a.Hm - 1) * a.os + a.oy0 < a.Hout && (a.Wm - 1) * a.os + a.ox0 < a.Wout, "disc_conv: a launch outside its frame");
    hipLaunchKernelGGL(k_disc_conv_mfma, dim3((a.Hm * a.Wm + 255) / 256, a.Cout / 64, B), dim3(NT), 0, st, a);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

#define PS_TRY(expr)              \
    do {                          \
        const int _rc = (expr);   \
        if (_rc != PS_OK) return _rc; \
    } while (0)

}  // namespace

extern "C" {

const char *ps_disc_conv_last_error(void) { return ps::last_error_ref().c_str(); }

int ps_disc_conv_takes(int B, int Ci, int Co, int H, int W, int stride, int pad) { return sizes_ok(B, Ci, Co, H, W, stride, pad) ? 1 : 0; }

size_t ps_disc_conv_workspace_bytes(int B, int Ci, int Co, int H, int W, int stride, int pad)
{
    if (!sizes_ok(B, Ci, Co, H, W, stride, pad)) return 0;
    return make_plan(B, Ci, Co, H, W, stride, pad).bytes;
}

int ps_disc_conv_parts(int B, int Ci, int Co, int H, int W, int stride, int pad)
{
    if (!sizes_ok(B, Ci, Co, H, W, stride, pad)) return 0;
    return make_plan(B, Ci, Co, H, W, stride, pad).parts;
}

int ps_disc_conv_forward_f16x3(const float *x, const float *weight, int B, int Ci, int Co, int H, int W, int stride, int pad, float *y,
                               int *overflow, void *workspace, size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(x && weight && y && overflow && workspace, "disc_conv_forward: null pointer");
    PS_REQUIRE(sizes_ok(B, Ci, Co, H, W, stride, pad), "disc_conv_forward: B = %d, Ci = %d, Co = %d, H = %d, W = %d, stride = %d, pad = %d: "
               "stride 1 or 2, pad 2, Ci and Co multiples of 64 up to 512, frames within 32-bit offsets required", B, Ci, Co, H, W, stride, pad);
    const Plan p = make_plan(B, Ci, Co, H, W, stride, pad);
    PS_REQUIRE(workspace_bytes >= p.bytes, "disc_conv_forward: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    PS_REQUIRE((uintptr_t)workspace % 256 == 0 && (uintptr_t)x % 4 == 0 && (uintptr_t)weight % 4 == 0 && (uintptr_t)y % 4 == 0,
               "disc_conv_forward: the workspace must be aligned to 256 bytes, the tensors to 4");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    float *amax = (float *)(ws + p.o_amax), *wscale2 = (float *)(ws + p.o_wscale);
    _Float16 *wp = (_Float16 *)(ws + p.o_wp), *xs = (_Float16 *)(ws + p.o_xs);
    PS_TRY(amax_scale(weight, p.n_wp, amax, wscale2, st));
    PS_TRY(pack_weight(weight, wscale2, 0, Co, Ci, wp, overflow, st));
    PS_TRY(to_nhwc(x, nullptr, B, Ci, H, W, pad, xs, p.n_xs, overflow, st));
    ConvArgs a;
    a.in_hi = xs; a.in_lo = xs + p.n_xs; a.w_hi = wp; a.w_lo = wp + p.n_wp; a.wscale2 = wscale2; a.gscale2 = nullptr; a.out = y;
    a.Hp = p.Hp; a.Wp = p.Wp; a.Cin = Ci; a.Cout = Co; a.Hout = p.Ho; a.Wout = p.Wo; a.Hm = p.Ho; a.Wm = p.Wo;
    a.s = stride; a.off = 0; a.KH = 4; a.KW = 4; a.os = 1; a.oy0 = 0; a.ox0 = 0;
    return launch_conv(a, B, st);
}

int ps_disc_conv_backward_f16x3(const float *x, const float *weight, const float *g, int B, int Ci, int Co, int H, int W, int stride,
                                int pad, float *grad_x, float *grad_weight, float *scale2, int *overflow, int *grad_overflow,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(x && weight && g && scale2 && overflow && grad_overflow && workspace, "disc_conv_backward: null pointer");
    PS_REQUIRE(sizes_ok(B, Ci, Co, H, W, stride, pad), "disc_conv_backward: B = %d, Ci = %d, Co = %d, H = %d, W = %d, stride = %d, pad = %d: "
               "stride 1 or 2, pad 2, Ci and Co multiples of 64 up to 512, frames within 32-bit offsets required", B, Ci, Co, H, W, stride, pad);
    const Plan p = make_plan(B, Ci, Co, H, W, stride, pad);
    PS_REQUIRE(workspace_bytes >= p.bytes, "disc_conv_backward: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    PS_REQUIRE((uintptr_t)workspace % 256 == 0 && (uintptr_t)x % 4 == 0 && (uintptr_t)weight % 4 == 0 && (uintptr_t)g % 4 == 0
               && (uintptr_t)grad_x % 4 == 0 && (uintptr_t)grad_weight % 4 == 0 && (uintptr_t)scale2 % 4 == 0,
               "disc_conv_backward: the workspace must be aligned to 256 bytes, the tensors to 4");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    float *amax = (float *)(ws + p.o_amax), *wscale2 = (float *)(ws + p.o_wscale);
    PS_TRY(amax_scale(g, (size_t)B * Co * p.Ho * p.Wo, amax, scale2, st));
    if (grad_x) {
        _Float16 *wp = (_Float16 *)(ws + p.o_wp), *gn = (_Float16 *)(ws + p.o_gn);
        PS_TRY(amax_scale(weight, p.n_wp, amax, wscale2, st));
        PS_TRY(pack_weight(weight, wscale2, stride == 1 ? 1 : 2, Co, Ci, wp, grad_overflow, st));
        PS_TRY(to_nhwc(g, scale2, B, Co, p.Ho, p.Wo, 1, gn, p.n_gn, grad_overflow, st));
        ConvArgs a;
        a.in_hi = gn; a.in_lo = gn + p.n_gn; a.wscale2 = wscale2; a.gscale2 = scale2; a.out = grad_x;
        a.Hp = p.Ho + 2; a.Wp = p.Wo + 2; a.Cin = Co; a.Cout = Ci; a.Hout = H; a.Wout = W; a.s = 1;
        if (stride == 1) {
            a.w_hi = wp; a.w_lo = wp + p.n_wp;
            a.Hm = H; a.Wm = W; a.off = 0; a.KH = 4; a.KW = 4; a.os = 1; a.oy0 = 0; a.ox0 = 0;
            PS_TRY(launch_conv(a, B, st));
        } else {
            for (int par = 0; par < 4; ++par) {
                const int py = par >> 1, px = par & 1;
                a.w_hi = wp + (size_t)4 * par * Co * Ci; a.w_lo = a.w_hi + p.n_wp;
                a.Hm = (H - py + 1) / 2; a.Wm = (W - px + 1) / 2; a.off = 1; a.KH = 2; a.KW = 2; a.os = 2; a.oy0 = py; a.ox0 = px;
                PS_TRY(launch_conv(a, B, st));
            }
        }
    }
    if (grad_weight) {
        _Float16 *gt = (_Float16 *)(ws + p.o_gt), *xt = (_Float16 *)(ws + p.o_xt);
        float *part = (float *)(ws + p.o_part);
        hipLaunchKernelGGL(k_disc_conv_rows, dim3(stream_grid(p.n_gt / 8)), dim3(NT), 0, st, g, (const float *)scale2, (size_t)B * Co, p.Ho, p.Wo,
                           p.Ho, 0, 1, 1, p.Wo, p.nch, gt, gt + p.n_gt, grad_overflow);
        PS_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_disc_conv_rows, dim3(stream_grid(p.n_xt / 8)), dim3(NT), 0, st, x, (const float *)nullptr, (size_t)B * Ci, H, W,
                           p.Hp, pad, stride, 4, p.Wo, p.nch, xt, xt + p.n_xt, overflow);
        PS_LAUNCH_CHECK();
        GwArgs a;
        a.g_hi = gt; a.g_lo = gt + p.n_gt; a.x_hi = xt; a.x_lo = xt + p.n_xt; a.part = part;
        a.B = B; a.Ci = Ci; a.Co = Co; a.Ho = p.Ho; a.Hp = p.Hp; a.Wo8 = p.Wo8; a.nch = p.nch; a.Q = p.Q; a.spf = p.spf; a.steps = p.steps;
        a.chunk = p.chunk; a.s = stride; a.ncib = Ci / 32;
        hipLaunchKernelGGL(k_disc_conv_gw_parts, dim3(p.parts, p.blocks), dim3(NT), 0, st, a);
        PS_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_disc_conv_gw_sum, dim3((unsigned)((p.n_wp + NT - 1) / NT)), dim3(NT), 0, st, (const float *)part, p.parts, Co, Ci,
                           (const float *)scale2, grad_weight);
        PS_LAUNCH_CHECK();
    }
    return PS_OK;
}

}  // extern "C"
