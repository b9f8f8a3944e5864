// unet_train.hip -- the elementwise half of the depth regressor (networks/architectures.py: Unet) in training for gfx950 (MI355X): plain
// nn.BatchNorm2d on the batch's statistics with a leaky ReLU written beside it, and relu -> bilinear x2 of the concatenation of two
// tensors, each with its backward pass.  Behind the C ABI of include/pixelsynth_unet_train.h (libpixelsynth_unet_train.so, beside
// libpixelsynth_hip.so whose set of exports it leaves as it is).
//
// The batch norm is norm_train.hip's design without the per-sample gain: every pass over the activation is a bandwidth pass over
// channels-last memory, 16 bytes per lane.  Workgroup (part, chunk) takes part p -- consecutive rows, the split of the header -- and up to
// 64 float4s of channels; its 256 threads are `rl` row lanes of `cw` channel quads (C / 4 need not divide 256: the threads left over idle).
//
//   k_stats          sum x and sum x^2 per thread in fp64 in ascending row, the row lanes added in ascending order through LDS, one row
//                    of the partial slab per part.  k_stats_finish: one thread per channel adds the slab's rows in ascending part,
//                    computes mean / var / rstd and updates the module's running statistics and its batch counter.
//   k_apply          y = x * scale - shift, z = leaky(y) beside it.
//   k_bwd_sums       per part the fp64 sums of g and g * xhat with g = dy + dz * leaky'(y) formed in registers; k_bwd_finish adds the
//                    parts: dbias, dweight and the two per-channel constants of dx; k_bwd_dx the input's gradient, g formed again.
//   k_up2_fwd        one thread per output float4: the four clamped neighbours of the operand its channels lie in, relu, the weights.
//   k_up2_bwd        one thread per input float4 of one operand: the gather of the header over at most 4 x 4 outputs, masked.
// No atomics: every sum has one fixed order.
#include "ps_common.h"

#include "../../include/pixelsynth_unet_train.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int MAX_CW = 64;                      // float4s of channels a workgroup takes

struct Plan {
    int C4, cw, rl, chunks, part_rows, parts;
    size_t slab, k, bytes;                      // byte offsets into the workspace, and its size
};

inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

inline bool sizes_ok(int N, int C) { return N >= 1 && C >= 4 && C % 4 == 0 && C <= PS_UNET_TRAIN_MAX_C; }

// The split of the rows and the layout of the workspace: a function of the sizes alone
inline Plan make_plan(int N, int C)
{
    Plan p;
    p.C4 = C / 4;
    p.cw = p.C4 < MAX_CW ? p.C4 : MAX_CW;
    p.rl = THREADS / p.cw;
    p.chunks = (int)ceil_div(p.C4, p.cw);
    p.part_rows = (int)(PS_UNET_TRAIN_PART_ROWS * ceil_div(ceil_div(N, PS_UNET_TRAIN_PART_ROWS), PS_UNET_TRAIN_MAX_PARTS));
    p.parts = (int)ceil_div(N, p.part_rows);
    p.slab = 0;
    p.k = ps::align_up(p.slab + (size_t)p.parts * 2 * C * sizeof(double), 256);
    p.bytes = ps::align_up(p.k + (size_t)2 * C * sizeof(float), 256);
    return p;
}

struct Geo {                                    // what the kernels need of the plan
    int N, C4, cw, rl, part_rows;
};

inline Geo geo_of(const Plan &p, int N) { return Geo{N, p.C4, p.cw, p.rl, p.part_rows}; }

// This thread's share of workgroup (blockIdx.x = part, blockIdx.y = channel chunk): channel quad q, rows r0, r0 + rl, ... < r1 (64-bit:
// r + rl may pass 2^31 where N is close to it)
struct Lane {
    bool on;
    int q;
    long long r0, r1;
};

__device__ __forceinline__ Lane lane_of(const Geo &g)
{
    Lane l;
    const int t = threadIdx.x, lane_row = t / g.cw;
    l.q = blockIdx.y * g.cw + t % g.cw;
    l.on = lane_row < g.rl && l.q < g.C4;
    l.r0 = (long long)blockIdx.x * g.part_rows + lane_row;
    const long long end = ((long long)blockIdx.x + 1) * g.part_rows;
    l.r1 = end < g.N ? end : g.N;
    return l;
}

struct Affine {
    f32x4 scale, shift;
};

__device__ __forceinline__ Affine affine_of(const f32x4 *__restrict__ mean, const f32x4 *__restrict__ rstd, const f32x4 *__restrict__ weight,
                                            const f32x4 *__restrict__ bias, int q)
{
    Affine a;
    a.scale = rstd[q] * weight[q];
    a.shift = mean[q] * a.scale - bias[q];
    return a;
}

// (-ffp-contract=off: a product and a difference)
__device__ __forceinline__ f32x4 norm_value(f32x4 x, f32x4 scale, f32x4 shift) { return x * scale - shift; }

// z of y: a NaN y fails y > 0 and slope * NaN is a NaN
__device__ __forceinline__ float leaky(float y, float slope) { return y > 0.0f ? y : slope * y; }

// g = dy + dz * leaky'(y): the term of a gradient that is absent is not added (no 0 + ...: -0 and NaN * 0 stay out)
__device__ __forceinline__ float grad_of(float y, float dy, float dz, bool has_dy, bool has_dz, float slope)
{
    const float through = y > 0.0f ? dz : dz * slope;
    return has_dy ? (has_dz ? dy + through : dy) : through;
}

// The eight fp64 sums of every thread (a[0..3], b[0..3]: its four channels' two sums) -> row `p` of the slab, (2, C) doubles: the row
// lanes of a channel are added in ascending order.  sh: THREADS * 8 doubles, [sum][thread]
__device__ __forceinline__ void lanes_to_slab(const double *a, const double *b, const Geo &g, int C, double *sh, double *__restrict__ slab)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        sh[k * THREADS + t] = a[k];
        sh[(4 + k) * THREADS + t] = b[k];
    }
    __syncthreads();
    double *out = slab + (size_t)blockIdx.x * 2 * C;
    for (int e = t; e < g.cw * 8; e += THREADS) {
        const int k = e / g.cw, qq = e % g.cw, q = blockIdx.y * g.cw + qq;
        if (q >= g.C4) continue;
        double s = 0.0;
        for (int lr = 0; lr < g.rl; ++lr) s += sh[k * THREADS + lr * g.cw + qq];
        out[(size_t)(k >> 2) * C + 4 * q + (k & 3)] = s;
    }
}

__global__ __launch_bounds__(THREADS) void k_stats(const f32x4 *__restrict__ x, Geo g, int C, double *__restrict__ slab)
{
    __shared__ double sh[THREADS * 8];
    const Lane l = lane_of(g);
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    if (l.on) {
#pragma unroll 4
        for (long long r = l.r0; r < l.r1; r += g.rl) {
            const f32x4 v = x[(size_t)r * g.C4 + l.q];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double e = (double)v[k];
                s1[k] += e;
                s2[k] += e * e;
            }
        }
    }
    lanes_to_slab(s1, s2, g, C, sh, slab);
}

// One thread per channel: the parts in ascending order
__global__ __launch_bounds__(THREADS) void k_stats_finish(const double *__restrict__ slab, int parts, int C, double n, float eps, float keep,
                                                          float momentum, float unbias, float *__restrict__ running_mean,
                                                          float *__restrict__ running_var, long long *__restrict__ tracked,
                                                          float *__restrict__ mean, float *__restrict__ var, float *__restrict__ rstd)
{
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int p = 0; p < parts; ++p) {
        s1 += slab[(size_t)p * 2 * C + c];
        s2 += slab[(size_t)p * 2 * C + C + c];
    }
    const double m = s1 / n, d = s2 / n - m * m;
    const float mf = (float)m, vf = (float)(d < 0.0 ? 0.0 : d);           // (a NaN stays one)
    const float ve = vf + eps;
    mean[c] = mf;
    var[c] = vf;
    rstd[c] = (float)(1.0 / sqrt((double)ve));
    if (running_mean) {
        running_mean[c] = running_mean[c] * keep + mf * momentum;
        running_var[c] = running_var[c] * keep + (vf * unbias) * momentum;
        if (c == 0) *tracked += 1;
    }
}

__global__ __launch_bounds__(THREADS) void k_apply(const f32x4 *__restrict__ x, const f32x4 *__restrict__ mean, const f32x4 *__restrict__ rstd,
                                                   const f32x4 *__restrict__ weight, const f32x4 *__restrict__ bias, Geo g, float slope,
                                                   f32x4 *__restrict__ y, f32x4 *__restrict__ z)
{
    const Lane l = lane_of(g);
    if (!l.on) return;
    const Affine a = affine_of(mean, rstd, weight, bias, l.q);
#pragma unroll 4
    for (long long r = l.r0; r < l.r1; r += g.rl) {
        const size_t i = (size_t)r * g.C4 + l.q;
        const f32x4 o = norm_value(x[i], a.scale, a.shift);
        y[i] = o;
        if (z) {
            f32x4 act;
#pragma unroll
            for (int k = 0; k < 4; ++k) act[k] = leaky(o[k], slope);
            z[i] = act;
        }
    }
}

__global__ __launch_bounds__(THREADS) void k_bwd_sums(const f32x4 *__restrict__ x, const f32x4 *__restrict__ dy, const f32x4 *__restrict__ dz,
                                                      const f32x4 *__restrict__ mean, const f32x4 *__restrict__ rstd,
                                                      const f32x4 *__restrict__ weight, const f32x4 *__restrict__ bias, Geo g, int C,
                                                      float slope, double *__restrict__ slab)
{
    __shared__ double sh[THREADS * 8];
    const Lane l = lane_of(g);
    double sg[4] = {0.0, 0.0, 0.0, 0.0}, sgx[4] = {0.0, 0.0, 0.0, 0.0};
    if (l.on) {
        const Affine a = affine_of(mean, rstd, weight, bias, l.q);
        const f32x4 m = mean[l.q], rs = rstd[l.q], zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
        for (long long r = l.r0; r < l.r1; r += g.rl) {
            const size_t i = (size_t)r * g.C4 + l.q;
            const f32x4 v = x[i], gy = dy ? dy[i] : zero, gz = dz ? dz[i] : zero;
            const f32x4 o = norm_value(v, a.scale, a.shift), xhat = (v - m) * rs;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double gk = (double)grad_of(o[k], gy[k], gz[k], dy != nullptr, dz != nullptr, slope);
                sg[k] += gk;
                sgx[k] += gk * (double)xhat[k];
            }
        }
    }
    lanes_to_slab(sg, sgx, g, C, sh, slab);
}

// One thread per channel: the parts in ascending order; dbias / dweight rounded once, and k[c] = weight * sum g / N, k[C + c] =
// weight * sum g xhat / N in fp64, rounded once
__global__ __launch_bounds__(THREADS) void k_bwd_finish(const double *__restrict__ slab, int parts, int C, double n, const float *__restrict__ weight,
                                                        float *__restrict__ dweight, float *__restrict__ dbias, float *__restrict__ k)
{
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int p = 0; p < parts; ++p) {
        s1 += slab[(size_t)p * 2 * C + c];
        s2 += slab[(size_t)p * 2 * C + C + c];
    }
    dbias[c] = (float)s1;
    dweight[c] = (float)s2;
    const double w = (double)weight[c];
    k[c] = (float)(w * s1 / n);
    k[C + c] = (float)(w * s2 / n);
}

__global__ __launch_bounds__(THREADS) void k_bwd_dx(const f32x4 *__restrict__ x, const f32x4 *__restrict__ dy, const f32x4 *__restrict__ dz,
                                                    const f32x4 *__restrict__ mean, const f32x4 *__restrict__ rstd,
                                                    const f32x4 *__restrict__ weight, const f32x4 *__restrict__ bias,
                                                    const f32x4 *__restrict__ k, Geo g, float slope, f32x4 *__restrict__ dx)
{
    const Lane l = lane_of(g);
    if (!l.on) return;
    const Affine a = affine_of(mean, rstd, weight, bias, l.q);
    const f32x4 m = mean[l.q], rs = rstd[l.q], w = weight[l.q], k1 = k[l.q], k2 = k[g.C4 + l.q], zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
    for (long long r = l.r0; r < l.r1; r += g.rl) {
        const size_t i = (size_t)r * g.C4 + l.q;
        const f32x4 v = x[i], gy = dy ? dy[i] : zero, gz = dz ? dz[i] : zero;
        const f32x4 o = norm_value(v, a.scale, a.shift), xhat = (v - m) * rs;
        f32x4 gr;
#pragma unroll
        for (int c = 0; c < 4; ++c) gr[c] = grad_of(o[c], gy[c], gz[c], dy != nullptr, dz != nullptr, slope);
        dx[i] = rs * (w * gr - k1 - xhat * k2);
    }
}

// ---- relu -> bilinear x2 of cat(a, b) ---------------------------------------------------------------------------------------------------
// bilinear x2, align_corners = False, the rule of nets.hip's up_src restated: source coordinate (d + 0.5) / 2 - 0.5, clamped at 0; the
// two source samples and the weight of the second one
__device__ __forceinline__ void up_src(int d, int n, int &i0, int &i1, float &w1)
{
    const float s = fmaxf((d + 0.5f) * 0.5f - 0.5f, 0.0f);
    i0 = (int)s;
    i1 = min(i0 + 1, n - 1);
    w1 = s - (float)i0;
}

// One axis of the adjoint, block_train.hip's up_axis restated: the (at most four) output indices 2 i - 1 .. 2 i + 2 that input index i of
// n hears from, their weights, and which of them exist
struct UpAxis {
    bool on[4];
    float w[4];
};

__device__ __forceinline__ UpAxis up_axis(int i, int n)
{
    UpAxis a;
    a.on[0] = i >= 1, a.w[0] = 0.25f;
    a.on[1] = true, a.w[1] = i > 0 ? 0.75f : 1.0f;
    a.on[2] = true, a.w[2] = i == n - 1 ? 1.0f : 0.75f;
    a.on[3] = i <= n - 2, a.w[3] = 0.25f;
    return a;
}

__global__ __launch_bounds__(THREADS) void k_up2_fwd(const f32x4 *__restrict__ a, const f32x4 *__restrict__ b, int H, int W, int Ca4, int Cb4,
                                                     size_t total4, f32x4 *__restrict__ out)
{
    const size_t e = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= total4) return;
    const int C4 = Ca4 + Cb4, c4 = (int)(e % C4);
    size_t p = e / C4;
    const int xo = (int)(p % (2 * (size_t)W));
    p /= 2 * (size_t)W;
    const int yo = (int)(p % (2 * (size_t)H));
    const size_t f = p / (2 * (size_t)H);
    const bool first = c4 < Ca4;
    const int Cs4 = first ? Ca4 : Cb4;
    const f32x4 *src = (first ? a + c4 : b + (c4 - Ca4)) + f * H * W * Cs4;
    int y0, y1, x0, x1;
    float wy, wx;
    up_src(yo, H, y0, y1, wy);
    up_src(xo, W, x0, x1, wx);
    const f32x4 v00 = ps::relu_keep_nan(src[((size_t)y0 * W + x0) * Cs4]);
    if (H == 1 && W == 1) {                     // (the pixel four times, exactly: 0.75 r + 0.25 r need not be r)
        out[e] = v00;
        return;
    }
    const f32x4 v01 = ps::relu_keep_nan(src[((size_t)y0 * W + x1) * Cs4]), v10 = ps::relu_keep_nan(src[((size_t)y1 * W + x0) * Cs4]),
                v11 = ps::relu_keep_nan(src[((size_t)y1 * W + x1) * Cs4]);
    const float w00 = (1.0f - wy) * (1.0f - wx), w01 = (1.0f - wy) * wx, w10 = wy * (1.0f - wx), w11 = wy * wx;
    out[e] = v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11;
}

__global__ __launch_bounds__(THREADS) void k_up2_bwd(const f32x4 *__restrict__ g, const f32x4 *__restrict__ src, int H, int W, int C4, int c04,
                                                     int Cs4, size_t total4, f32x4 *__restrict__ out)
{
    const size_t e = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= total4) return;
    const int c4 = (int)(e % Cs4);
    size_t p = e / Cs4;
    const int x = (int)(p % W);
    p /= W;
    const int y = (int)(p % H);
    const size_t f = p / H;
    const UpAxis ay = up_axis(y, H), ax = up_axis(x, W);
    const f32x4 *gf = g + f * 4 * H * W * C4 + c04 + c4;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (!ay.on[r]) continue;
        const f32x4 *row = gf + (size_t)(2 * y - 1 + r) * 2 * W * C4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!ax.on[c]) continue;
            const float w = ay.w[r] * ax.w[c];
            acc = acc + row[(size_t)(2 * x - 1 + c) * C4] * w;
        }
    }
    const f32x4 s = src[e];
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = s[k] > 0.0f ? acc[k] : (s[k] != s[k] ? s[k] : 0.0f);
    out[e] = o;
}

using ps::aligned16;

// Workgroups of 256 threads over total4 items, one each; 0 where that is more than a grid holds
inline unsigned blocks_for(size_t total4)
{
    const size_t blocks = (total4 + THREADS - 1) / THREADS;
    return blocks <= 0x7fffffffull ? (unsigned)blocks : 0u;
}

}  // namespace

extern "C" {

const char *ps_unet_train_last_error(void) { return ps::last_error_ref().c_str(); }

size_t ps_unet_train_workspace_bytes(int N, int C)
{
    if (!sizes_ok(N, C)) return 0;
    return make_plan(N, C).bytes;
}

int ps_unet_train_parts(int N, int C)
{
    if (!sizes_ok(N, C)) return 0;
    return make_plan(N, C).parts;
}

#define UNET_TRAIN_SIZES(what)                                                                                                        \
    PS_REQUIRE(N >= 1 && C >= 1, what ": N = %d, C = %d, expected both >= 1", N, C);                                                  \
    PS_REQUIRE(C % 4 == 0, what ": C = %d is not a multiple of 4", C);                                                                \
    PS_REQUIRE(C <= PS_UNET_TRAIN_MAX_C, what ": C = %d, more than %d channels", C, PS_UNET_TRAIN_MAX_C)

#define UNET_TRAIN_WORKSPACE(what, need)                                                                                              \
    PS_REQUIRE(workspace, what ": null pointer (workspace)");                                                                         \
    PS_REQUIRE(workspace_bytes >= (need), what ": workspace of %zu bytes, %zu needed", workspace_bytes, (size_t)(need));              \
    PS_REQUIRE(aligned16(workspace), what ": the workspace must be aligned to 16 bytes")

int ps_bn_stats_f32(const float *x, int N, int C, float eps, float momentum, float *running_mean, float *running_var,
                    long long *num_batches_tracked, float *mean, float *var, float *rstd, void *workspace, size_t workspace_bytes,
                    void *stream)
{
    PS_REQUIRE(x && mean && var && rstd, "bn_stats: null pointer");
    UNET_TRAIN_SIZES("bn_stats");
    PS_REQUIRE(!running_mean == !running_var && !running_mean == !num_batches_tracked,
               "bn_stats: running_mean, running_var and num_batches_tracked go together");
    PS_REQUIRE(!running_mean || N >= 2, "bn_stats: N = %d, the running variance needs N >= 2", N);
    PS_REQUIRE(aligned16(x) && aligned16(running_mean) && aligned16(running_var) && aligned16(mean) && aligned16(var) && aligned16(rstd) &&
                   ((uintptr_t)num_batches_tracked & 7) == 0,
               "bn_stats: every buffer must be aligned to 16 bytes (num_batches_tracked to 8)");
    const Plan p = make_plan(N, C);
    UNET_TRAIN_WORKSPACE("bn_stats", p.bytes);
    hipStream_t st = (hipStream_t)stream;
    double *slab = (double *)((char *)workspace + p.slab);
    hipLaunchKernelGGL(k_stats, dim3(p.parts, p.chunks), dim3(THREADS), 0, st, (const f32x4 *)x, geo_of(p, N), C, slab);
    PS_LAUNCH_CHECK();
    const float keep = (float)(1.0 - (double)momentum), unbias = N >= 2 ? (float)((double)N / ((double)N - 1.0)) : 1.0f;
    hipLaunchKernelGGL(k_stats_finish, dim3((unsigned)ceil_div(C, THREADS)), dim3(THREADS), 0, st, slab, p.parts, C, (double)N, eps, keep,
                       momentum, unbias, running_mean, running_var, num_batches_tracked, mean, var, rstd);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_bn_act_apply_f32(const float *x, const float *mean, const float *rstd, const float *weight, const float *bias, int N, int C,
                        float slope, float *y, float *z, void *stream)
{
    PS_REQUIRE(x && mean && rstd && weight && bias && y, "bn_act_apply: null pointer");
    UNET_TRAIN_SIZES("bn_act_apply");
    PS_REQUIRE(aligned16(x) && aligned16(mean) && aligned16(rstd) && aligned16(weight) && aligned16(bias) && aligned16(y) && aligned16(z),
               "bn_act_apply: every buffer must be aligned to 16 bytes");
    const Plan p = make_plan(N, C);
    hipLaunchKernelGGL(k_apply, dim3(p.parts, p.chunks), dim3(THREADS), 0, (hipStream_t)stream, (const f32x4 *)x, (const f32x4 *)mean,
                       (const f32x4 *)rstd, (const f32x4 *)weight, (const f32x4 *)bias, geo_of(p, N), slope, (f32x4 *)y, (f32x4 *)z);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_bn_act_backward_f32(const float *x, const float *dy, const float *dz, const float *mean, const float *rstd, const float *weight,
                           const float *bias, int N, int C, float slope, float *dx, float *dweight, float *dbias, void *workspace,
                           size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(x && mean && rstd && weight && bias && dweight && dbias, "bn_act_backward: null pointer");
    PS_REQUIRE(dy || dz, "bn_act_backward: null pointer (dy and dz)");
    UNET_TRAIN_SIZES("bn_act_backward");
    PS_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(dz) && aligned16(mean) && aligned16(rstd) && aligned16(weight) && aligned16(bias) &&
                   aligned16(dx) && aligned16(dweight) && aligned16(dbias),
               "bn_act_backward: every buffer must be aligned to 16 bytes");
    const Plan p = make_plan(N, C);
    UNET_TRAIN_WORKSPACE("bn_act_backward", p.bytes);
    hipStream_t st = (hipStream_t)stream;
    double *slab = (double *)((char *)workspace + p.slab);
    float *k = (float *)((char *)workspace + p.k);
    const Geo g = geo_of(p, N);
    const f32x4 *x4 = (const f32x4 *)x, *dy4 = (const f32x4 *)dy, *dz4 = (const f32x4 *)dz, *mean4 = (const f32x4 *)mean,
                *rstd4 = (const f32x4 *)rstd, *w4 = (const f32x4 *)weight, *b4 = (const f32x4 *)bias;
    hipLaunchKernelGGL(k_bwd_sums, dim3(p.parts, p.chunks), dim3(THREADS), 0, st, x4, dy4, dz4, mean4, rstd4, w4, b4, g, C, slope, slab);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bwd_finish, dim3((unsigned)ceil_div(C, THREADS)), dim3(THREADS), 0, st, slab, p.parts, C, (double)N, weight, dweight,
                       dbias, k);
    PS_LAUNCH_CHECK();
    if (!dx) return PS_OK;
    hipLaunchKernelGGL(k_bwd_dx, dim3(p.parts, p.chunks), dim3(THREADS), 0, st, x4, dy4, dz4, mean4, rstd4, w4, b4, (const f32x4 *)k, g, slope,
                       (f32x4 *)dx);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

#define UP2_SIZES(what)                                                                                                               \
    PS_REQUIRE(B >= 1 && H >= 1 && W >= 1, what ": B = %d, H = %d, W = %d, expected all >= 1", B, H, W);                              \
    PS_REQUIRE(H < (1 << 30) && W < (1 << 30), what ": frame too large")

int ps_relu_up2_cat_f32(const float *a, const float *b, int B, int H, int W, int Ca, int Cb, float *out, void *stream)
{
    PS_REQUIRE(a && out, "relu_up2_cat: null pointer");
    UP2_SIZES("relu_up2_cat");
    PS_REQUIRE(Ca >= 4 && Ca % 4 == 0 && Cb >= 0 && Cb % 4 == 0 && Ca <= PS_UNET_TRAIN_MAX_C && Cb <= PS_UNET_TRAIN_MAX_C,
               "relu_up2_cat: Ca = %d, Cb = %d: multiples of 4, Ca >= 4 required", Ca, Cb);
    PS_REQUIRE((b != nullptr) == (Cb > 0), "relu_up2_cat: b goes with Cb > 0");
    PS_REQUIRE(aligned16(a) && aligned16(b) && aligned16(out), "relu_up2_cat: buffers must be aligned to 16 bytes");
    const size_t total4 = (size_t)B * 4 * H * W * ((Ca + Cb) / 4);
    const unsigned blocks = blocks_for(total4);
    PS_REQUIRE(blocks, "relu_up2_cat: too many elements for one launch");
    hipLaunchKernelGGL(k_up2_fwd, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, (const f32x4 *)a, (const f32x4 *)b, H, W, Ca / 4, Cb / 4,
                       total4, (f32x4 *)out);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_relu_up2_cat_backward_f32(const float *g, const float *src, int B, int H, int W, int C, int c0, int Cs, float *grad_in,
                                 void *stream)
{
    PS_REQUIRE(g && src && grad_in, "relu_up2_cat_backward: null pointer");
    UP2_SIZES("relu_up2_cat_backward");
    PS_REQUIRE(C >= 4 && C % 4 == 0 && C <= 2 * PS_UNET_TRAIN_MAX_C && Cs >= 4 && Cs % 4 == 0 && c0 >= 0 && c0 % 4 == 0 && c0 + Cs <= C,
               "relu_up2_cat_backward: C = %d, c0 = %d, Cs = %d: multiples of 4 with c0 + Cs <= C required", C, c0, Cs);
    PS_REQUIRE(aligned16(g) && aligned16(src) && aligned16(grad_in), "relu_up2_cat_backward: buffers must be aligned to 16 bytes");
    const size_t total4 = (size_t)B * H * W * (Cs / 4);
    const unsigned blocks = blocks_for(total4);
    PS_REQUIRE(blocks && blocks_for((size_t)B * 4 * H * W * (C / 4)), "relu_up2_cat_backward: too many elements for one launch");
    hipLaunchKernelGGL(k_up2_bwd, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, (const f32x4 *)g, (const f32x4 *)src, H, W, C / 4, c0 / 4,
                       Cs / 4, total4, (f32x4 *)grad_in);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
