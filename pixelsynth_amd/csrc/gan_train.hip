// gan_train.hip -- what touches an activation-sized tensor when the multiscale discriminator trains, besides its 4 x 4 convolutions, for
// gfx950 (MI355X): instance normalisation + LeakyReLU forward and backward (the InstanceNorm2d + LeakyReLU pairs of model1..3,
// models/networks/discriminators.py:97-114) and the feature-matching L1 over the intermediate maps forward and backward
// (compute_generator_loss, models/losses/gan_loss.py:199-214), which torch autograd runs as a dozen passes and eight small launch chains.
//
// Behind the C ABI of include/pixelsynth_gan_train.h (libpixelsynth_gan_train.so, beside libpixelsynth_hip.so whose set of exports it
// leaves as it is).  Tensors are NCHW as torch's convolutions leave them, so a plane is contiguous and fits a wavefront or a workgroup:
//
//   k_norm_fwd / k_norm_bwd <LANES, NV>     LANES = 64: a wavefront per plane, four planes per workgroup, no barrier; LANES = 256: a
//                                           workgroup per plane.  A thread holds NV values of the plane (and of dy) in registers between
//                                           the reduction and the elementwise phase: one read, one write.
//   k_norm_fwd_stream / k_norm_bwd_stream   planes past PS_GAN_TRAIN_RESIDENT_HW: a workgroup per plane, two passes.
//   k_feat_tiles, k_feat_finish             |f - r| per tile of every map in one launch, then the tiles of each map in ascending order.
//   k_feat_bwd                              s_k sgn(f - r) into the fake halves, +0 into the real ones, one launch.
// Plane bases are aligned to 4 bytes only (HW is odd at the network's sizes): every access is a dword, consecutive across lanes.
// No atomics: every sum has one fixed order (a thread's values ascending, the lanes of a wavefront as a butterfly, wavefronts ascending).
#include "ps_common.h"

#include "../../include/pixelsynth_gan_train.h"

namespace {

constexpr int THREADS = 256, WAVE = 64, WAVES = THREADS / WAVE;
constexpr int MAX_NV = 32;                      // values a thread holds at the most
constexpr int MAX_MAPS = PS_GAN_TRAIN_MAX_MAPS;
constexpr long long TILE = PS_GAN_TRAIN_TILE;
constexpr long long MAX_HALF = 1ll << 40;

static_assert(PS_GAN_TRAIN_WAVE_HW == WAVE * MAX_NV && PS_GAN_TRAIN_RESIDENT_HW == THREADS * MAX_NV, "the forms of the header");

struct Sum2 {
    double a, b;
};

// Every lane gets the sum over the wavefront, the same bits in each: lane ^ 1, ^ 2, ... ^ 32
__device__ __forceinline__ Sum2 wave_sum(Sum2 s)
{
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        const double a = __shfl_xor(s.a, m, WAVE), b = __shfl_xor(s.b, m, WAVE);
        s.a += a;
        s.b += b;
    }
    return s;
}

// The sum over the LANES threads that share a plane; LANES = 256: once per kernel (one use of `red`), by every thread of the workgroup
template <int LANES> __device__ __forceinline__ Sum2 group_sum(Sum2 s, double (*red)[WAVES])
{
    s = wave_sum(s);
    if (LANES == WAVE) return s;
    const int w = threadIdx.x / WAVE;
    if (threadIdx.x % WAVE == 0) {
        red[0][w] = s.a;
        red[1][w] = s.b;
    }
    __syncthreads();
    Sum2 r = {red[0][0], red[1][0]};
#pragma unroll
    for (int i = 1; i < WAVES; ++i) {
        r.a += red[0][i];
        r.b += red[1][i];
    }
    return r;
}

struct Stats {
    float mean, rstd;
};

__device__ __forceinline__ Stats stats_of(Sum2 s, int HW, float eps)
{
    const double n = (double)HW, m = s.a / n;
    double var = s.b / n - m * m;
    var = var < 0.0 ? 0.0 : var;                // (a NaN stays)
    const float ve = (float)var + eps;
    return Stats{(float)m, (float)(1.0 / sqrt((double)ve))};
}

// The two fp32 steps every kernel that needs v takes (-ffp-contract=off: a difference, a product)
__device__ __forceinline__ float norm_value(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.0f ? v : v * slope; }
__device__ __forceinline__ float grad_through(float v, float dy, float slope) { return v > 0.0f ? dy : dy * slope; }
__device__ __forceinline__ float grad_in(float g, float v, float m1, float m2, float rstd) { return rstd * ((g - m1) - v * m2); }

// This thread's plane and its lane in it; off: a wavefront past the last plane (LANES = 64 only: the grid of LANES = 256 is the planes)
template <int LANES> __device__ __forceinline__ bool plane_of(int planes, long long &plane, int &t)
{
    plane = (long long)blockIdx.x * (THREADS / LANES) + threadIdx.x / LANES;
    t = threadIdx.x % LANES;
    return plane < planes;
}

template <int LANES, int NV>
__global__ __launch_bounds__(THREADS) void k_norm_fwd(const float *__restrict__ x, int planes, int HW, float eps, float slope,
                                                      float *__restrict__ y, float *__restrict__ mean, float *__restrict__ rstd)
{
    __shared__ double red[2][WAVES];
    long long plane;
    int t;
    if (!plane_of<LANES>(planes, plane, t)) return;
    const float *px = x + (size_t)plane * HW;
    float v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int idx = t + i * LANES;
        v[i] = idx < HW ? px[idx] : 0.0f;
    }
    Sum2 s = {0.0, 0.0};
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const double d = (double)v[i];
        s.a += d;
        s.b += d * d;
    }
    const Stats st = stats_of(group_sum<LANES>(s, red), HW, eps);
    if (t == 0) {
        mean[plane] = st.mean;
        rstd[plane] = st.rstd;
    }
    float *py = y + (size_t)plane * HW;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int idx = t + i * LANES;
        if (idx < HW) py[idx] = lrelu(norm_value(v[i], st.mean, st.rstd), slope);
    }
}

template <int LANES, int NV>
__global__ __launch_bounds__(THREADS) void k_norm_bwd(const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ mean,
                                                      const float *__restrict__ rstd, int planes, int HW, float slope, float *__restrict__ dx)
{
    __shared__ double red[2][WAVES];
    long long plane;
    int t;
    if (!plane_of<LANES>(planes, plane, t)) return;
    const size_t base = (size_t)plane * HW;
    const float m = mean[plane], rs = rstd[plane];
    float v[NV], g[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int idx = t + i * LANES;
        v[i] = idx < HW ? x[base + idx] : 0.0f;
        g[i] = idx < HW ? dy[base + idx] : 0.0f;
    }
    Sum2 s = {0.0, 0.0};
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int idx = t + i * LANES;
        v[i] = norm_value(v[i], m, rs);
        g[i] = grad_through(v[i], g[i], slope);
        if (idx < HW) {                         // (past the plane v is not 0: (0 - mean) * rstd)
            s.a += (double)g[i];
            s.b += (double)g[i] * (double)v[i];
        }
    }
    s = group_sum<LANES>(s, red);
    const float m1 = (float)(s.a / (double)HW), m2 = (float)(s.b / (double)HW);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int idx = t + i * LANES;
        if (idx < HW) dx[base + idx] = grad_in(g[i], v[i], m1, m2, rs);
    }
}

// Planes past the resident forms: a workgroup per plane, thread t takes t, t + 256, ... in both passes (the second finds most of a
// plane of this size in the cache; it is a second read all the same)
__global__ __launch_bounds__(THREADS) void k_norm_fwd_stream(const float *__restrict__ x, int HW, float eps, float slope, float *__restrict__ y,
                                                             float *__restrict__ mean, float *__restrict__ rstd)
{
    __shared__ double red[2][WAVES];
    const size_t base = (size_t)blockIdx.x * HW;
    const int t = threadIdx.x;
    Sum2 s = {0.0, 0.0};
    for (long long i = t; i < HW; i += THREADS) {
        const double d = (double)x[base + i];
        s.a += d;
        s.b += d * d;
    }
    const Stats st = stats_of(group_sum<THREADS>(s, red), HW, eps);
    if (t == 0) {
        mean[blockIdx.x] = st.mean;
        rstd[blockIdx.x] = st.rstd;
    }
    for (long long i = t; i < HW; i += THREADS) y[base + i] = lrelu(norm_value(x[base + i], st.mean, st.rstd), slope);
}

__global__ __launch_bounds__(THREADS) void k_norm_bwd_stream(const float *__restrict__ x, const float *__restrict__ dy,
                                                             const float *__restrict__ mean, const float *__restrict__ rstd, int HW,
                                                             float slope, float *__restrict__ dx)
{
    __shared__ double red[2][WAVES];
    const size_t base = (size_t)blockIdx.x * HW;
    const int t = threadIdx.x;
    const float m = mean[blockIdx.x], rs = rstd[blockIdx.x];
    Sum2 s = {0.0, 0.0};
    for (long long i = t; i < HW; i += THREADS) {
        const float v = norm_value(x[base + i], m, rs), g = grad_through(v, dy[base + i], slope);
        s.a += (double)g;
        s.b += (double)g * (double)v;
    }
    s = group_sum<THREADS>(s, red);
    const float m1 = (float)(s.a / (double)HW), m2 = (float)(s.b / (double)HW);
    for (long long i = t; i < HW; i += THREADS) {
        const float v = norm_value(x[base + i], m, rs), g = grad_through(v, dy[base + i], slope);
        dx[base + i] = grad_in(g, v, m1, m2, rs);
    }
}

// ---- feature matching ------------------------------------------------------------------------------------------------------------------

// The maps of a call, passed by value: tile `first[k]` is the first of map k, first[n_maps] the number of tiles
struct MapTable {
    const float *p[MAX_MAPS];
    long long n[MAX_MAPS];
    double w[MAX_MAPS];
    unsigned first[MAX_MAPS + 1];
};

struct GradTable {
    float *g[MAX_MAPS];
};

// The map of tile blockIdx.x (the same for every thread), the tile's first value in a half and its length
struct TileOf {
    int k;
    long long at;
    int len;
};

__device__ __forceinline__ TileOf tile_of(const MapTable &T, int n_maps)
{
    TileOf o;
    o.k = 0;
    while (o.k + 1 < n_maps && blockIdx.x >= T.first[o.k + 1]) ++o.k;
    o.at = (long long)(blockIdx.x - T.first[o.k]) * TILE;
    const long long left = T.n[o.k] - o.at;
    o.len = (int)(left < TILE ? left : TILE);
    return o;
}

__global__ __launch_bounds__(THREADS) void k_feat_tiles(MapTable T, int n_maps, double *__restrict__ partial)
{
    __shared__ double red[2][WAVES];
    const TileOf o = tile_of(T, n_maps);
    const float *f = T.p[o.k] + o.at, *r = f + T.n[o.k];
    Sum2 s = {0.0, 0.0};
#pragma unroll 8
    for (int i = threadIdx.x; i < o.len; i += THREADS) s.a += (double)fabsf(f[i] - r[i]);
    s = group_sum<THREADS>(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s.a;
}

// One workgroup: the tiles of each map in ascending order (staged 256 at a time, added by one thread), then the maps in ascending order
__global__ __launch_bounds__(THREADS) void k_feat_finish(MapTable T, int n_maps, const double *__restrict__ partial,
                                                         float *__restrict__ per_map, float *__restrict__ total)
{
    __shared__ double stage[THREADS];
    const int t = threadIdx.x;
    double tot = 0.0;
    for (int k = 0; k < n_maps; ++k) {
        double S = 0.0;
        for (unsigned c = T.first[k]; c < T.first[k + 1]; c += THREADS) {
            const unsigned m = T.first[k + 1] - c < (unsigned)THREADS ? T.first[k + 1] - c : (unsigned)THREADS;
            __syncthreads();
            if ((unsigned)t < m) stage[t] = partial[c + t];
            __syncthreads();
            if (t == 0)
                for (unsigned j = 0; j < m; ++j) S += stage[j];
        }
        if (t == 0) {
            const double mean = S / (double)T.n[k];
            per_map[k] = (float)mean;
            tot += T.w[k] * mean;
        }
    }
    if (t == 0) total[0] = (float)tot;
}

__global__ __launch_bounds__(THREADS) void k_feat_bwd(MapTable T, GradTable G, int n_maps, const float *__restrict__ grad_total)
{
    const TileOf o = tile_of(T, n_maps);
    const long long n = T.n[o.k];
    const float s = (float)((double)grad_total[0] * T.w[o.k] / (double)n);
    const float *f = T.p[o.k] + o.at, *r = f + n;
    float *gf = G.g[o.k] + o.at, *gr = gf + n;
#pragma unroll 8
    for (int i = threadIdx.x; i < o.len; i += THREADS) {
        const float d = f[i] - r[i];
        gf[i] = s * (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : d));        // (d is +-0 or not a number in the last branch)
        gr[i] = 0.0f;
    }
}

// -> the number of tiles, 0 for sizes the entry points refuse; fills T.n and T.first
inline long long lay_out(const long long *half_elems, int n_maps, MapTable &T)
{
    if (!half_elems || n_maps < 1 || n_maps > MAX_MAPS) return 0;
    long long tiles = 0;
    for (int k = 0; k < n_maps; ++k) {
        if (half_elems[k] < 1 || half_elems[k] >= MAX_HALF) return 0;
        T.n[k] = half_elems[k];
        T.first[k] = (unsigned)tiles;
        tiles += (half_elems[k] + TILE - 1) / TILE;
        if (tiles >= (1ll << 31)) return 0;
    }
    for (int k = n_maps; k <= MAX_MAPS; ++k) T.first[k] = (unsigned)tiles;
    for (int k = n_maps; k < MAX_MAPS; ++k) {
        T.n[k] = 0;
        T.p[k] = nullptr;
        T.w[k] = 0.0;
    }
    return tiles;
}

#define NV_CASES(K, LANES, nv, ...)                                                                                                     \
    switch (nv) {                                                                                                                       \
    case 4: hipLaunchKernelGGL((K<LANES, 4>), __VA_ARGS__); break;                                                                      \
    case 8: hipLaunchKernelGGL((K<LANES, 8>), __VA_ARGS__); break;                                                                      \
    case 12: hipLaunchKernelGGL((K<LANES, 12>), __VA_ARGS__); break;                                                                    \
    case 16: hipLaunchKernelGGL((K<LANES, 16>), __VA_ARGS__); break;                                                                    \
    case 20: hipLaunchKernelGGL((K<LANES, 20>), __VA_ARGS__); break;                                                                    \
    case 24: hipLaunchKernelGGL((K<LANES, 24>), __VA_ARGS__); break;                                                                    \
    case 28: hipLaunchKernelGGL((K<LANES, 28>), __VA_ARGS__); break;                                                                    \
    default: hipLaunchKernelGGL((K<LANES, 32>), __VA_ARGS__); break;                                                                    \
    }

// Values a thread of `lanes` holds of a plane of HW <= 32 lanes values: the multiple of 4 that covers it
inline int values_per_thread(int HW, int lanes) { return 4 * (((HW + lanes - 1) / lanes + 3) / 4); }

}  // namespace

extern "C" {

const char *ps_gan_train_last_error(void) { return ps::last_error_ref().c_str(); }

int ps_in_lrelu_forward_f32(const float *x, int planes, int HW, float eps, float slope, float *y, float *mean, float *rstd,
                            void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace, (void)workspace_bytes;
    PS_REQUIRE(x && y && mean && rstd, "in_lrelu_forward: null pointer");
    PS_REQUIRE(planes >= 1 && HW >= 1, "in_lrelu_forward: planes = %d, HW = %d, expected both >= 1", planes, HW);
    hipStream_t st = (hipStream_t)stream;
    if (HW <= PS_GAN_TRAIN_WAVE_HW) {
        const dim3 grid((unsigned)((planes + WAVES - 1) / WAVES));
        NV_CASES(k_norm_fwd, WAVE, values_per_thread(HW, WAVE), grid, dim3(THREADS), 0, st, x, planes, HW, eps, slope, y, mean, rstd);
    } else if (HW <= PS_GAN_TRAIN_RESIDENT_HW) {
        NV_CASES(k_norm_fwd, THREADS, values_per_thread(HW, THREADS), dim3(planes), dim3(THREADS), 0, st, x, planes, HW, eps, slope, y, mean,
                 rstd);
    } else {
        hipLaunchKernelGGL(k_norm_fwd_stream, dim3(planes), dim3(THREADS), 0, st, x, HW, eps, slope, y, mean, rstd);
    }
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_in_lrelu_backward_f32(const float *x, const float *dy, const float *mean, const float *rstd, int planes, int HW, float slope,
                             float *dx, void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace, (void)workspace_bytes;
    PS_REQUIRE(x && dy && mean && rstd && dx, "in_lrelu_backward: null pointer");
    PS_REQUIRE(planes >= 1 && HW >= 1, "in_lrelu_backward: planes = %d, HW = %d, expected both >= 1", planes, HW);
    hipStream_t st = (hipStream_t)stream;
    if (HW <= PS_GAN_TRAIN_WAVE_HW) {
        const dim3 grid((unsigned)((planes + WAVES - 1) / WAVES));
        NV_CASES(k_norm_bwd, WAVE, values_per_thread(HW, WAVE), grid, dim3(THREADS), 0, st, x, dy, mean, rstd, planes, HW, slope, dx);
    } else if (HW <= PS_GAN_TRAIN_RESIDENT_HW) {
        NV_CASES(k_norm_bwd, THREADS, values_per_thread(HW, THREADS), dim3(planes), dim3(THREADS), 0, st, x, dy, mean, rstd, planes, HW, slope,
                 dx);
    } else {
        hipLaunchKernelGGL(k_norm_bwd_stream, dim3(planes), dim3(THREADS), 0, st, x, dy, mean, rstd, HW, slope, dx);
    }
    PS_LAUNCH_CHECK();
    return PS_OK;
}

size_t ps_gan_feat_workspace_bytes(const long long *half_elems, int n_maps)
{
    MapTable T;
    return ps::align_up((size_t)lay_out(half_elems, n_maps, T) * sizeof(double), 256);
}

#define GAN_FEAT_TABLE(what)                                                                                                          \
    PS_REQUIRE(maps && half_elems && weights, what ": null pointer");                                                                 \
    PS_REQUIRE(n_maps >= 1 && n_maps <= MAX_MAPS, what ": n_maps = %d, expected 1 .. %d", n_maps, MAX_MAPS);                           \
    MapTable T;                                                                                                                       \
    const long long tiles = lay_out(half_elems, n_maps, T);                                                                           \
    PS_REQUIRE(tiles > 0, what ": a map of fewer than 1 or of 2^40 values or more per half, or 2^31 tiles or more");                  \
    for (int k = 0; k < n_maps; ++k) {                                                                                                \
        PS_REQUIRE(maps[k], what ": null pointer (map %d)", k);                                                                       \
        T.p[k] = maps[k];                                                                                                             \
        T.w[k] = weights[k];                                                                                                          \
    }

int ps_gan_feat_l1_f32(const float *const *maps, const long long *half_elems, const double *weights, int n_maps, float *per_map,
                       float *total, void *workspace, size_t workspace_bytes, void *stream)
{
    GAN_FEAT_TABLE("gan_feat_l1");
    PS_REQUIRE(per_map && total, "gan_feat_l1: null pointer");
    PS_REQUIRE(workspace, "gan_feat_l1: null pointer (workspace)");
    PS_REQUIRE(workspace_bytes >= (size_t)tiles * sizeof(double), "gan_feat_l1: workspace of %zu bytes, %zu needed", workspace_bytes,
               (size_t)tiles * sizeof(double));
    PS_REQUIRE(ps::aligned16(workspace), "gan_feat_l1: the workspace must be aligned to 16 bytes");
    hipStream_t st = (hipStream_t)stream;
    double *partial = (double *)workspace;
    hipLaunchKernelGGL(k_feat_tiles, dim3((unsigned)tiles), dim3(THREADS), 0, st, T, n_maps, partial);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_feat_finish, dim3(1), dim3(THREADS), 0, st, T, n_maps, (const double *)partial, per_map, total);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_gan_feat_l1_backward_f32(const float *const *maps, const long long *half_elems, const double *weights, int n_maps,
                                const float *grad_total, float *const *grads, void *stream)
{
    GAN_FEAT_TABLE("gan_feat_l1_backward");
    PS_REQUIRE(grad_total && grads, "gan_feat_l1_backward: null pointer");
    GradTable G;
    for (int k = 0; k < MAX_MAPS; ++k) {
        PS_REQUIRE(k >= n_maps || grads[k], "gan_feat_l1_backward: null pointer (gradient of map %d)", k);
        G.g[k] = k < n_maps ? grads[k] : nullptr;
    }
    hipLaunchKernelGGL(k_feat_bwd, dim3((unsigned)tiles), dim3(THREADS), 0, (hipStream_t)stream, T, G, n_maps, grad_total);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
