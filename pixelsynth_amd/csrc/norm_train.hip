// norm_train.hip -- the noise-conditioned batch norm of the refinement decoder in training mode for gfx950 (MI355X): the batch statistics
// and the update of the stored ones, the normalisation + ReLU on them, and the backward pass (the reference's bn.forward in training
// mode, models/layers/normalization.py:114-200, which torch autograd runs as about a dozen full passes over the activation).
//
// Behind the C ABI of include/pixelsynth_norm_train.h (libpixelsynth_norm_train.so, beside libpixelsynth_hip.so whose set of exports it
// leaves as it is).  Every pass over the activation is a bandwidth pass over channels-last memory, 16 bytes per lane, and all of them
// walk it the same way (lane_of): workgroup (p, chunk) takes part p -- consecutive rows of ONE frame, the split of the header -- and up
// to 64 float4s of channels; its 256 threads are `rl` row lanes of `cw` channel quads, C / 4 need not divide 256 (the threads left over
// idle).  A thread keeps its four channels' constants in registers and walks rows r0 + lane, + rl, + 2 rl, ..., four at a time, the next
// four's loads issued before the current four are used.
//
//   k_stats          sum x and sum x^2 per thread in fp64 in ascending row, the row lanes added in ascending order through LDS, one
//                    row of the partial slab per part.  k_stats_finish adds the slab's rows in ascending part (staged through LDS:
//                    sum_parts), computes mean / var / rstd and updates the stored statistics.
//   k_apply          y = x * scale - shift (+ ReLU): norm_value, the one inline function every kernel that needs v calls.
//   k_bwd_sums       per part the fp64 sums of g and g * xhat, as k_stats; k_bwd_frames adds each frame's parts: dbias, dgain;
//                    k_bwd_channels the two per-channel means over ascending b; k_bwd_dx the input's gradient.
// No atomics: every sum has one fixed order.
#include "ps_common.h"

#include "../../include/pixelsynth_norm_train.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int MAX_CW = 64;                      // float4s of channels a workgroup takes
constexpr int DEPTH = 4;                        // rows a thread has in flight
constexpr int FIN_CH = 32, FIN_COLS = 2 * FIN_CH;                 // channels of a finishing workgroup; their columns of the slab (two sums each)
constexpr int FIN_PARTS = 64, FIN_LANES = THREADS / FIN_COLS, FIN_PER = FIN_PARTS / FIN_LANES;    // parts staged at a time

struct Plan {
    int C4, cw, rl, chunks, part_rows, ppf, parts;
    size_t slab, frames, k, bytes;              // byte offsets into the workspace, and its size
};

inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

inline bool sizes_ok(int B, int HW, int C)
{
    return B >= 1 && HW >= 1 && C >= 1 && C % 4 == 0 && C <= PS_NORM_TRAIN_MAX_C && (long long)HW * C < (1ll << 31) &&
           (long long)B * HW < (1ll << 31);
}

// The split of the rows and the layout of the workspace: a function of the sizes alone
inline Plan make_plan(int B, int HW, int C)
{
    Plan p;
    p.C4 = C / 4;
    p.cw = p.C4 < MAX_CW ? p.C4 : MAX_CW;
    p.rl = THREADS / p.cw;
    p.chunks = (int)ceil_div(p.C4, p.cw);
    const long long per_frame = PS_NORM_TRAIN_MAX_PARTS / B > 1 ? PS_NORM_TRAIN_MAX_PARTS / B : 1;
    p.part_rows = (int)(PS_NORM_TRAIN_PART_ROWS * ceil_div(ceil_div(HW, PS_NORM_TRAIN_PART_ROWS), per_frame));
    p.ppf = (int)ceil_div(HW, p.part_rows);
    p.parts = B * p.ppf;                        // (B <= 2^31 / HW and ppf <= HW / 512 + 1: fits)
    p.slab = 0;
    p.frames = ps::align_up(p.slab + (size_t)p.parts * 2 * C * sizeof(double), 256);
    p.k = ps::align_up(p.frames + (size_t)B * 2 * C * sizeof(double), 256);
    p.bytes = ps::align_up(p.k + (size_t)2 * C * sizeof(float), 256);
    return p;
}

struct Geo {                                    // what the kernels need of the plan
    int HW, C4, cw, rl, part_rows, ppf;
};

inline Geo geo_of(const Plan &p, int HW) { return Geo{HW, p.C4, p.cw, p.rl, p.part_rows, p.ppf}; }

// This thread's share of workgroup (blockIdx.x = part, blockIdx.y = channel chunk): frame b, channel quad q, rows r0, r0 + rl, ... < r1
struct Lane {
    bool on;
    int b, q, r0, r1;
};

__device__ __forceinline__ Lane lane_of(const Geo &g)
{
    Lane l;
    const int t = threadIdx.x, p = blockIdx.x, pf = p % g.ppf, lane_row = t / g.cw;
    l.b = p / g.ppf;
    l.q = blockIdx.y * g.cw + t % g.cw;
    l.on = lane_row < g.rl && l.q < g.C4;
    l.r0 = pf * g.part_rows + lane_row;
    l.r1 = min((pf + 1) * g.part_rows, g.HW);
    return l;
}

// The normalisation as the reference's fused_bn writes it, in its order (-ffp-contract=off: a product and a difference)
__device__ __forceinline__ f32x4 norm_value(f32x4 x, f32x4 scale, f32x4 shift) { return x * scale - shift; }

struct Affine {
    f32x4 scale, shift;
};

__device__ __forceinline__ Affine affine_of(const f32x4 *__restrict__ mean, const f32x4 *__restrict__ rstd, const f32x4 *__restrict__ gain,
                                            const f32x4 *__restrict__ bias, int b, int q, int C4)
{
    Affine a;
    a.scale = rstd[q] * gain[(size_t)b * C4 + q];
    a.shift = mean[q] * a.scale - bias[(size_t)b * C4 + q];
    return a;
}

// What the ReLU lets through of dy where the forward's value was v.  v not a number: the gradient is not one either (the forward's
// ps::relu_keep_nan kept the NaN; a clean 0 here would hide it)
__device__ __forceinline__ float grad_through(float v, float dy, bool relu)
{
    if (!relu) return dy;
    return v > 0.0f ? dy : (v != v ? v : 0.0f);
}

// The walk: this lane's rows in ascending order, DEPTH rows at a time: load(s, d, i) for each of them into set s of the caller's two
// register sets, i the row's float4 index, and use(s, d, i) for each -- the next DEPTH rows' loads are issued before the current ones
// are used, so a wave has loads in flight while it computes
template <typename Load, typename Use>
__device__ __forceinline__ void walk(const Lane &l, const Geo &g, size_t base, Load load, Use use)
{
    const int step = DEPTH * g.rl, last = (DEPTH - 1) * g.rl;
    int r = l.r0;
    auto load_rows = [&](int s, int from) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) load(s, d, base + (size_t)(from + d * g.rl) * g.C4);
    };
    auto use_rows = [&](int s, int from) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) use(s, d, base + (size_t)(from + d * g.rl) * g.C4);
    };
    if (r + last < l.r1) {
        load_rows(0, r);
        for (;;) {
            bool more = r + step + last < l.r1;
            if (more) load_rows(1, r + step);
            use_rows(0, r);
            r += step;
            if (!more) break;
            more = r + step + last < l.r1;
            if (more) load_rows(0, r + step);
            use_rows(1, r);
            r += step;
            if (!more) break;
        }
    }
    for (; r < l.r1; r += g.rl) {
        load(0, 0, base + (size_t)r * g.C4);
        use(0, 0, base + (size_t)r * g.C4);
    }
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
        const size_t base = (size_t)l.b * g.HW * g.C4 + l.q;
        f32x4 v[2][DEPTH];
        walk(l, g, base, [&](int s, int d, size_t i) { v[s][d] = x[i]; }, [&](int s, int d, size_t) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double e = (double)v[s][d][k];
                s1[k] += e;
                s2[k] += e * e;
            }
        });
    }
    lanes_to_slab(s1, s2, g, C, sh, slab);
}

// The sum over parts p0 .. p1 - 1, in that order, of column `col` of the slab (ncols doubles per part) -- for the FIN_COLS columns of
// a workgroup at once: thread t asks for the column of j = t & 63 (col < 0: none) and the threads t < 64 get the answer.  FIN_PARTS
// parts at a time are fetched by all 256 threads into LDS (the next batch while this one is added), where one thread per column adds them.
__device__ __forceinline__ double sum_parts(const double *__restrict__ slab, size_t ncols, long long col, int p0, int p1, double *sh)
{
    const int t = threadIdx.x, j = t & (FIN_COLS - 1), pl = t / FIN_COLS;
    double acc = 0.0, v[FIN_PER];
    auto fetch = [&](int base) {
#pragma unroll
        for (int u = 0; u < FIN_PER; ++u) {
            const int p = base + u * FIN_LANES + pl;
            v[u] = col >= 0 && p < p1 ? slab[(size_t)p * ncols + (size_t)col] : 0.0;
        }
    };
    fetch(p0);
    for (int base = p0; base < p1; base += FIN_PARTS) {
        __syncthreads();                                                   // (the previous batch has been added)
#pragma unroll
        for (int u = 0; u < FIN_PER; ++u) sh[(u * FIN_LANES + pl) * FIN_COLS + j] = v[u];
        __syncthreads();
        fetch(base + FIN_PARTS);                                           // (past p1: zeros, no load)
        if (pl == 0) {
            const int n = min(FIN_PARTS, p1 - base);
            for (int i = 0; i < n; ++i) acc += sh[i * FIN_COLS + j];
        }
    }
    return acc;
}

// The column of the slab thread t of a finishing workgroup adds: j < 32 the first sum of channel c0 + j, else the second of c0 + j - 32
__device__ __forceinline__ long long fin_col(int C, int block)
{
    const int j = threadIdx.x & (FIN_COLS - 1), c = block * FIN_CH + (j & (FIN_CH - 1));
    return c < C ? (long long)(j / FIN_CH) * C + c : -1;
}

__global__ __launch_bounds__(THREADS) void k_stats_finish(const double *__restrict__ slab, int parts, int C, double n, float eps, float keep,
                                                          float momentum, const float *__restrict__ pend, float *__restrict__ stored_mean,
                                                          float *__restrict__ stored_var, float *__restrict__ mean, float *__restrict__ var,
                                                          float *__restrict__ rstd)
{
    __shared__ double sh[FIN_PARTS * FIN_COLS];
    __shared__ double tot[FIN_COLS];
    const int t = threadIdx.x;
    const double s = sum_parts(slab, (size_t)2 * C, fin_col(C, blockIdx.x), 0, parts, sh);
    if (t < FIN_COLS) tot[t] = s;
    __syncthreads();
    const int c = blockIdx.x * FIN_CH + t;
    if (t >= FIN_CH || c >= C) return;
    const double m = tot[t] / n, d = tot[FIN_CH + t] / n - m * m;
    const float mf = (float)m, vf = (float)(d < 0.0 ? 0.0 : d);           // (a NaN stays one)
    const float ve = vf + eps;
    mean[c] = mf;
    var[c] = vf;
    rstd[c] = (float)(1.0 / sqrt((double)ve));
    const float shifted = pend ? mf + pend[c] : mf;
    stored_mean[c] = stored_mean[c] * keep + shifted * momentum;
    stored_var[c] = stored_var[c] * keep + vf * momentum;
}

__global__ __launch_bounds__(THREADS) void k_apply(const f32x4 *__restrict__ x, const f32x4 *__restrict__ mean, const f32x4 *__restrict__ rstd,
                                                   const f32x4 *__restrict__ gain, const f32x4 *__restrict__ bias, Geo g, int relu,
                                                   f32x4 *__restrict__ y)
{
    const Lane l = lane_of(g);
    if (!l.on) return;
    const Affine a = affine_of(mean, rstd, gain, bias, l.b, l.q, g.C4);
    const size_t base = (size_t)l.b * g.HW * g.C4 + l.q;
    f32x4 v[2][DEPTH];
    walk(l, g, base, [&](int s, int d, size_t i) { v[s][d] = x[i]; }, [&](int s, int d, size_t i) {
        const f32x4 o = norm_value(v[s][d], a.scale, a.shift);
        y[i] = relu ? ps::relu_keep_nan(o) : o;
    });
}

__global__ __launch_bounds__(THREADS) void k_bwd_sums(const f32x4 *__restrict__ x, const f32x4 *__restrict__ dy, const f32x4 *__restrict__ mean,
                                                      const f32x4 *__restrict__ rstd, const f32x4 *__restrict__ gain,
                                                      const f32x4 *__restrict__ bias, Geo g, int C, int relu, double *__restrict__ slab)
{
    __shared__ double sh[THREADS * 8];
    const Lane l = lane_of(g);
    double sg[4] = {0.0, 0.0, 0.0, 0.0}, sgx[4] = {0.0, 0.0, 0.0, 0.0};
    if (l.on) {
        const Affine a = affine_of(mean, rstd, gain, bias, l.b, l.q, g.C4);
        const f32x4 m = mean[l.q], rs = rstd[l.q];
        const size_t base = (size_t)l.b * g.HW * g.C4 + l.q;
        f32x4 v[2][DEPTH], w[2][DEPTH];
        walk(l, g, base, [&](int s, int d, size_t i) { v[s][d] = x[i]; w[s][d] = dy[i]; }, [&](int s, int d, size_t) {
            const f32x4 o = norm_value(v[s][d], a.scale, a.shift), xhat = (v[s][d] - m) * rs;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double gk = (double)grad_through(o[k], w[s][d][k], relu);
                sg[k] += gk;
                sgx[k] += gk * (double)xhat[k];
            }
        });
    }
    lanes_to_slab(sg, sgx, g, C, sh, slab);
}

// grid (B, channels / 32): the frame's parts added in ascending order; dbias / dgain rounded once, the fp64 sums kept for k_bwd_channels
__global__ __launch_bounds__(THREADS) void k_bwd_frames(const double *__restrict__ slab, int ppf, int C, double *__restrict__ frames,
                                                        float *__restrict__ dgain, float *__restrict__ dbias)
{
    __shared__ double sh[FIN_PARTS * FIN_COLS];
    const int t = threadIdx.x, b = blockIdx.x;
    const long long col = fin_col(C, blockIdx.y);
    const double s = sum_parts(slab, (size_t)2 * C, col, b * ppf, (b + 1) * ppf, sh);
    if (t >= FIN_COLS || col < 0) return;
    frames[(size_t)b * 2 * C + col] = s;
    const int c = blockIdx.y * FIN_CH + (t & (FIN_CH - 1));
    (t < FIN_CH ? dbias : dgain)[(size_t)b * C + c] = (float)s;
}

// One thread per channel: k[c] = sum_b gain * (sum g) / N, k[C + c] = sum_b gain * (sum g xhat) / N, ascending b in fp64
__global__ __launch_bounds__(THREADS) void k_bwd_channels(const double *__restrict__ frames, const float *__restrict__ gain, int B, int C,
                                                          double n, float *__restrict__ k)
{
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= C) return;
    double k1 = 0.0, k2 = 0.0;
    for (int b = 0; b < B; ++b) {
        const double gn = (double)gain[(size_t)b * C + c];
        k1 += gn * frames[(size_t)b * 2 * C + c];
        k2 += gn * frames[(size_t)b * 2 * C + C + c];
    }
    k[c] = (float)(k1 / n);
    k[C + c] = (float)(k2 / n);
}

__global__ __launch_bounds__(THREADS) void k_bwd_dx(const f32x4 *__restrict__ x, const f32x4 *__restrict__ dy, const f32x4 *__restrict__ mean,
                                                    const f32x4 *__restrict__ rstd, const f32x4 *__restrict__ gain,
                                                    const f32x4 *__restrict__ bias, const f32x4 *__restrict__ k, Geo g, int relu,
                                                    f32x4 *__restrict__ dx)
{
    const Lane l = lane_of(g);
    if (!l.on) return;
    const Affine a = affine_of(mean, rstd, gain, bias, l.b, l.q, g.C4);
    const f32x4 m = mean[l.q], rs = rstd[l.q], gn = gain[(size_t)l.b * g.C4 + l.q], k1 = k[l.q], k2 = k[g.C4 + l.q];
    const size_t base = (size_t)l.b * g.HW * g.C4 + l.q;
    f32x4 v[2][DEPTH], w[2][DEPTH];
    walk(l, g, base, [&](int s, int d, size_t i) { v[s][d] = x[i]; w[s][d] = dy[i]; }, [&](int s, int d, size_t i) {
        const f32x4 o = norm_value(v[s][d], a.scale, a.shift), xhat = (v[s][d] - m) * rs;
        f32x4 gr;
#pragma unroll
        for (int c = 0; c < 4; ++c) gr[c] = grad_through(o[c], w[s][d][c], relu);
        dx[i] = rs * (gn * gr - k1 - xhat * k2);
    });
}

using ps::aligned16;

}  // namespace

extern "C" {

const char *ps_norm_train_last_error(void) { return ps::last_error_ref().c_str(); }

size_t ps_norm_train_workspace_bytes(int B, int HW, int C)
{
    if (!sizes_ok(B, HW, C)) return 0;
    return make_plan(B, HW, C).bytes;
}

int ps_norm_train_parts(int B, int HW, int C)
{
    if (!sizes_ok(B, HW, C)) return 0;
    return make_plan(B, HW, C).parts;
}

#define NORM_TRAIN_SIZES(what)                                                                                                        \
    PS_REQUIRE(B >= 1 && HW >= 1 && C >= 1, what ": B = %d, HW = %d, C = %d, expected all >= 1", B, HW, C);                           \
    PS_REQUIRE(C % 4 == 0, what ": C = %d is not a multiple of 4", C);                                                                \
    PS_REQUIRE(C <= PS_NORM_TRAIN_MAX_C, what ": C = %d, more than %d channels", C, PS_NORM_TRAIN_MAX_C);                              \
    PS_REQUIRE(sizes_ok(B, HW, C), what ": B = %d, HW = %d, C = %d: a frame of 2^31 elements or more, or 2^31 rows or more", B, HW, C)

#define NORM_TRAIN_WORKSPACE(what, need)                                                                                              \
    PS_REQUIRE(workspace, what ": null pointer (workspace)");                                                                         \
    PS_REQUIRE(workspace_bytes >= (need), what ": workspace of %zu bytes, %zu needed", workspace_bytes, (size_t)(need));              \
    PS_REQUIRE(aligned16(workspace), what ": the workspace must be aligned to 16 bytes")

int ps_norm_train_stats_f32(const float *x, const float *pend, int B, int HW, int C, float eps, float keep, float momentum,
                            float *stored_mean, float *stored_var, float *mean, float *var, float *rstd, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(x && stored_mean && stored_var && mean && var && rstd, "norm_train_stats: null pointer");
    NORM_TRAIN_SIZES("norm_train_stats");
    PS_REQUIRE(aligned16(x) && aligned16(pend) && aligned16(stored_mean) && aligned16(stored_var) && aligned16(mean) && aligned16(var) &&
                   aligned16(rstd),
               "norm_train_stats: every buffer must be aligned to 16 bytes");
    const Plan p = make_plan(B, HW, C);
    NORM_TRAIN_WORKSPACE("norm_train_stats", p.bytes);
    hipStream_t st = (hipStream_t)stream;
    double *slab = (double *)((char *)workspace + p.slab);
    hipLaunchKernelGGL(k_stats, dim3(p.parts, p.chunks), dim3(THREADS), 0, st, (const f32x4 *)x, geo_of(p, HW), C, slab);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_stats_finish, dim3((unsigned)ceil_div(C, FIN_CH)), dim3(THREADS), 0, st, slab, p.parts, C, (double)B * (double)HW,
                       eps, keep, momentum, pend, stored_mean, stored_var, mean, var, rstd);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_norm_train_apply_f32(const float *x, const float *mean, const float *rstd, const float *gain, const float *bias, int B, int HW,
                            int C, int relu, float *y, void *stream)
{
    PS_REQUIRE(x && mean && rstd && gain && bias && y, "norm_train_apply: null pointer");
    NORM_TRAIN_SIZES("norm_train_apply");
    PS_REQUIRE(aligned16(x) && aligned16(mean) && aligned16(rstd) && aligned16(gain) && aligned16(bias) && aligned16(y),
               "norm_train_apply: every buffer must be aligned to 16 bytes");
    const Plan p = make_plan(B, HW, C);
    hipLaunchKernelGGL(k_apply, dim3(p.parts, p.chunks), dim3(THREADS), 0, (hipStream_t)stream, (const f32x4 *)x, (const f32x4 *)mean,
                       (const f32x4 *)rstd, (const f32x4 *)gain, (const f32x4 *)bias, geo_of(p, HW), relu, (f32x4 *)y);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_norm_train_backward_f32(const float *x, const float *dy, const float *mean, const float *rstd, const float *gain,
                               const float *bias, int B, int HW, int C, int relu, float *dx, float *dgain, float *dbias,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(x && dy && mean && rstd && gain && bias && dgain && dbias, "norm_train_backward: null pointer");
    NORM_TRAIN_SIZES("norm_train_backward");
    PS_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(mean) && aligned16(rstd) && aligned16(gain) && aligned16(bias) && aligned16(dx) &&
                   aligned16(dgain) && aligned16(dbias),
               "norm_train_backward: every buffer must be aligned to 16 bytes");
    const Plan p = make_plan(B, HW, C);
    NORM_TRAIN_WORKSPACE("norm_train_backward", p.bytes);
    hipStream_t st = (hipStream_t)stream;
    double *slab = (double *)((char *)workspace + p.slab), *frames = (double *)((char *)workspace + p.frames);
    float *k = (float *)((char *)workspace + p.k);
    const Geo g = geo_of(p, HW);
    const f32x4 *x4 = (const f32x4 *)x, *dy4 = (const f32x4 *)dy, *mean4 = (const f32x4 *)mean, *rstd4 = (const f32x4 *)rstd,
                *gain4 = (const f32x4 *)gain, *bias4 = (const f32x4 *)bias;
    hipLaunchKernelGGL(k_bwd_sums, dim3(p.parts, p.chunks), dim3(THREADS), 0, st, x4, dy4, mean4, rstd4, gain4, bias4, g, C, relu, slab);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bwd_frames, dim3(B, (unsigned)ceil_div(C, FIN_CH)), dim3(THREADS), 0, st, slab, p.ppf, C, frames, dgain, dbias);
    PS_LAUNCH_CHECK();
    if (!dx) return PS_OK;
    hipLaunchKernelGGL(k_bwd_channels, dim3((unsigned)ceil_div(C, THREADS)), dim3(THREADS), 0, st, frames, gain, B, C,
                       (double)B * (double)HW, k);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bwd_dx, dim3(p.parts, p.chunks), dim3(THREADS), 0, st, x4, dy4, mean4, rstd4, gain4, bias4, (const f32x4 *)k, g, relu,
                       (f32x4 *)dx);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
