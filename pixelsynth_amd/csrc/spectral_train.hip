// spectral_train.hip -- the spectral normalisation of all layers of a network in training, forward and backward, for gfx950 (MI355X):
// torch's legacy torch.nn.utils.spectral_norm hook (n_power_iterations = 1, dim = 0) runs two to three dozen launches of a few
// microseconds per layer and forward + backward; here a TABLE of layers goes through five launches forward and two backward, whatever
// its length.
//
// Behind the C ABI of include/pixelsynth_spectral_train.h (libpixelsynth_spectral_train.so, beside libpixelsynth_hip.so whose set of
// exports it leaves as it is).  The table (sizes, offsets, the addresses of W / u / v) is filled on the host by ps_spectral_plan and
// lies on the device as well; a workgroup finds its layer by bisection of the table's prefix sums.
//
//   k_sn_wtu      a workgroup per (layer, part of PS_SPECTRAL_PART_ROWS rows): the part's share of W^T u, fp64, to the workspace
//   k_sn_v        a workgroup per layer: the parts ascending, t and |t| in fp64, v = fp32(t / max(|t|, eps)) in place and into v_saved
//   k_sn_wv       a wavefront per row: s = W v, fp64, to the workspace
//   k_sn_u        a workgroup per layer: |s| in fp64, u = fp32(s / max(|s|, eps)) in place and into u_saved, sigma = fp32(u . s)
//   k_sn_div      a workgroup per tile of PS_SPECTRAL_TILE values of all layers: W_sn = W / sigma
//   k_sn_dot      a workgroup per tile: the tile's share of sum G * W_sn, fp64
//   k_sn_dw       a workgroup per tile: d from its layer's tiles, then dW = (G - (d u_r) v_c) / sigma
// No atomics: every sum has one fixed order, a function of the layer's sizes alone (the header states them).  16-byte loads where a row or
// a tile allows them; the same thread adds the same values either way.
#include "ps_common.h"

#include <cstring>

#include "../../include/pixelsynth_spectral_train.h"

namespace {

constexpr int THREADS = 256, WAVE = 64, WAVES = THREADS / WAVE;
constexpr int MAX_LAYERS = PS_SPECTRAL_MAX_LAYERS, PART_ROWS = PS_SPECTRAL_PART_ROWS, TILE = PS_SPECTRAL_TILE;
constexpr unsigned MAGIC = 0x70735354u;         // "psST"

static_assert(TILE % (4 * THREADS) == 0, "a tile is whole rounds of four values per thread");

struct Layer {
    const float *W;
    float *u, *v;
    int R, C;
    int iterate;
    float eps;
    long long elem_off;         // of W_sn / dW, in values, a multiple of 4
    long long tu_off;           // of the parts of W^T u in the workspace, in doubles
    int row_off, col_off;       // of u_saved (and s in the workspace), of v_saved (a multiple of 4)
    int parts;
    int inter;                  // column m in memory is column (m % inter) * (C / inter) + m / inter of W; 1: the same
};

struct Table {
    unsigned magic, check;      // check: a hash of everything behind it; the kernels compare their image's with the host's
    int n_layers, total_parts, total_rowgroups, total_tiles;
    long long total_elems, total_rows, total_cols, total_tu;
    int first_part[MAX_LAYERS + 1], first_rowgroup[MAX_LAYERS + 1], first_tile[MAX_LAYERS + 1];
    int pad;
    Layer layer[MAX_LAYERS];
};

struct GradTable {
    const float *g[MAX_LAYERS];
};

// The layer of item b of a prefix table: the last k with first[k] <= b (first[0] = 0 <= b < first[n])
__device__ __forceinline__ int layer_of(const int *first, int n, int b)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (b >= first[mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Four values from p, of which the first m (1 .. 4) exist; the rest are zeros.  vec: p is aligned to 16 bytes and m == 4
__device__ __forceinline__ float4 load4(const float *p, bool vec, int m)
{
    if (vec) return *reinterpret_cast<const float4 *>(p);
    float4 r;
    r.x = p[0];
    r.y = m > 1 ? p[1] : 0.0f;
    r.z = m > 2 ? p[2] : 0.0f;
    r.w = m > 3 ? p[3] : 0.0f;
    return r;
}

__device__ __forceinline__ void store4(float *p, bool vec, int m, float4 r)
{
    if (vec) {
        *reinterpret_cast<float4 *>(p) = r;
        return;
    }
    p[0] = r.x;
    if (m > 1) p[1] = r.y;
    if (m > 2) p[2] = r.z;
    if (m > 3) p[3] = r.w;
}

__device__ __forceinline__ bool aligned16_dev(const void *p) { return ((uintptr_t)p & 15) == 0; }

// Every lane gets the sum over the wavefront, the same bits in each: lane ^ 1, ^ 2, ... ^ 32
__device__ __forceinline__ double wave_sum(double s)
{
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) s += __shfl_xor(s, m, WAVE);
    return s;
}

// The sum over the workgroup, in every thread: the wavefronts ascending.  Called by all 256 threads; may be called again (it
// synchronises before it writes)
__device__ __forceinline__ double block_sum(double s, double *red)
{
    s = wave_sum(s);
    __syncthreads();
    if (threadIdx.x % WAVE == 0) red[threadIdx.x / WAVE] = s;
    __syncthreads();
    double r = red[0];
#pragma unroll
    for (int i = 1; i < WAVES; ++i) r += red[i];
    return r;
}

// max(n, eps) that keeps a NaN (torch's clamp_min does; v_max_f32 would answer eps)
__device__ __forceinline__ double at_least(double n, double eps) { return n < eps ? eps : n; }

__global__ __launch_bounds__(THREADS) void k_sn_wtu(const Table *__restrict__ T, unsigned check, double *__restrict__ tu)
{
    const int b = blockIdx.x;
    if (T->check != check || b >= T->total_parts) return;
    const int l = layer_of(T->first_part, T->n_layers, b);
    const Layer L = T->layer[l];
    if (!L.iterate) return;
    const int p = b - T->first_part[l], r0 = p * PART_ROWS, r1 = min(L.R, r0 + PART_ROWS), C = L.C;
    const bool vec = C % 4 == 0 && aligned16_dev(L.W);
    double *out = tu + L.tu_off + (long long)p * C;
    for (int c = 4 * threadIdx.x; c < C; c += 4 * THREADS) {
        const int m = min(4, C - c);
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int r = r0; r < r1; ++r) {
            const double ur = (double)L.u[r];
            const float4 w = load4(L.W + (size_t)r * C + c, vec, m);
            a0 += (double)w.x * ur;
            a1 += (double)w.y * ur;
            a2 += (double)w.z * ur;
            a3 += (double)w.w * ur;
        }
        out[c] = a0;
        if (m > 1) out[c + 1] = a1;
        if (m > 2) out[c + 2] = a2;
        if (m > 3) out[c + 3] = a3;
    }
}

__global__ __launch_bounds__(THREADS) void k_sn_v(const Table *__restrict__ T, unsigned check, double *__restrict__ tu,
                                                  float *__restrict__ v_saved)
{
    __shared__ double red[WAVES];
    if (T->check != check || (int)blockIdx.x >= T->n_layers) return;
    const Layer L = T->layer[blockIdx.x];
    const int t = threadIdx.x, C = L.C;
    float *vs = v_saved + L.col_off;            // (in memory order; L.v in W's)
    const int inner = C / L.inter;
    if (!L.iterate) {
        for (int c = t; c < C; c += THREADS) vs[c] = L.v[(c % L.inter) * inner + c / L.inter];
        return;
    }
    double *parts = tu + L.tu_off;
    double q = 0.0;
    for (int c = t; c < C; c += THREADS) {
        double a = 0.0;
        for (int p = 0; p < L.parts; ++p) a += parts[(long long)p * C + c];
        parts[c] = a;                           // (t_c stays fp64, in part 0's place; read back below by the thread that wrote it)
        q += a * a;
    }
    q = block_sum(q, red);
    const double n = at_least(sqrt(q), (double)L.eps);
    for (int c = t; c < C; c += THREADS) {
        const float val = (float)(parts[c] / n);        // the one rounding of v_c
        vs[c] = val;
        L.v[(c % L.inter) * inner + c / L.inter] = val;
    }
}

__global__ __launch_bounds__(THREADS) void k_sn_wv(const Table *__restrict__ T, unsigned check, const float *__restrict__ v_saved,
                                                   double *__restrict__ s)
{
    const int b = blockIdx.x;
    if (T->check != check || b >= T->total_rowgroups) return;
    const int l = layer_of(T->first_rowgroup, T->n_layers, b);
    const Layer L = T->layer[l];
    const int row = (b - T->first_rowgroup[l]) * WAVES + threadIdx.x / WAVE, lane = threadIdx.x % WAVE, C = L.C;
    if (row >= L.R) return;                     // (a whole wavefront; no barrier follows)
    const bool vec = C % 4 == 0 && aligned16_dev(L.W);
    const float *w = L.W + (size_t)row * C, *vs = v_saved + L.col_off;
    double a = 0.0;
    for (int c = 4 * lane; c < C; c += 4 * WAVE) {
        const int m = min(4, C - c);
        const float4 x = load4(w + c, vec, m), y = load4(vs + c, m == 4, m);
        a += (double)x.x * (double)y.x;
        a += (double)x.y * (double)y.y;
        a += (double)x.z * (double)y.z;
        a += (double)x.w * (double)y.w;
    }
    a = wave_sum(a);
    if (lane == 0) s[L.row_off + row] = a;
}

__global__ __launch_bounds__(THREADS) void k_sn_u(const Table *__restrict__ T, unsigned check, const double *__restrict__ s,
                                                  float *__restrict__ u_saved, float *__restrict__ sigma)
{
    __shared__ double red[WAVES];
    if (T->check != check || (int)blockIdx.x >= T->n_layers) return;
    const Layer L = T->layer[blockIdx.x];
    const int t = threadIdx.x, R = L.R;
    const double *sl = s + L.row_off;
    float *us = u_saved + L.row_off;
    if (L.iterate) {
        double q = 0.0;
        for (int r = t; r < R; r += THREADS) q += sl[r] * sl[r];
        q = block_sum(q, red);
        const double n = at_least(sqrt(q), (double)L.eps);
        for (int r = t; r < R; r += THREADS) {
            const float val = (float)(sl[r] / n);       // the one rounding of u_r
            us[r] = val;
            L.u[r] = val;
        }
    } else {
        for (int r = t; r < R; r += THREADS) us[r] = L.u[r];
    }
    double dot = 0.0;
    for (int r = t; r < R; r += THREADS) dot += (double)us[r] * sl[r];      // (us[r]: this thread's own store)
    dot = block_sum(dot, red);
    if (t == 0) sigma[blockIdx.x] = (float)dot;
}

// The tile of blockIdx.x: its layer, its first value in the layer and its length
struct TileOf {
    int l, at, len;
};

__device__ __forceinline__ TileOf tile_of(const Table *T)
{
    TileOf o;
    o.l = layer_of(T->first_tile, T->n_layers, blockIdx.x);
    const int n = T->layer[o.l].R * T->layer[o.l].C;
    o.at = ((int)blockIdx.x - T->first_tile[o.l]) * TILE;
    o.len = min(TILE, n - o.at);
    return o;
}

__global__ __launch_bounds__(THREADS) void k_sn_div(const Table *__restrict__ T, unsigned check, const float *__restrict__ sigma,
                                                    float *__restrict__ w_sn)
{
    if (T->check != check || (int)blockIdx.x >= T->total_tiles) return;
    const TileOf o = tile_of(T);
    const Layer L = T->layer[o.l];
    const float sg = sigma[o.l];
    const float *src = L.W + o.at;
    float *dst = w_sn + L.elem_off + o.at;      // (aligned to 16 bytes: the base is, elem_off and the tile are multiples of 4)
    const bool vec = aligned16_dev(src);
    for (int i = 4 * threadIdx.x; i < o.len; i += 4 * THREADS) {
        const int m = min(4, o.len - i);
        float4 w = load4(src + i, vec && m == 4, m);
        w.x /= sg;
        w.y /= sg;
        w.z /= sg;
        w.w /= sg;
        store4(dst + i, m == 4, m, w);
    }
}

__global__ __launch_bounds__(THREADS) void k_sn_dot(const Table *__restrict__ T, unsigned check, GradTable G,
                                                    const float *__restrict__ w_sn, double *__restrict__ partial)
{
    __shared__ double red[WAVES];
    if (T->check != check || (int)blockIdx.x >= T->total_tiles) return;
    const TileOf o = tile_of(T);
    const float *g = G.g[o.l];
    double q = 0.0;
    if (g) {
        g += o.at;
        const float *w = w_sn + T->layer[o.l].elem_off + o.at;
        const bool vec = aligned16_dev(g);
        for (int i = 4 * threadIdx.x; i < o.len; i += 4 * THREADS) {
            const int m = min(4, o.len - i);
            const float4 x = load4(g + i, vec && m == 4, m), y = load4(w + i, m == 4, m);
            q += (double)x.x * (double)y.x;
            q += (double)x.y * (double)y.y;
            q += (double)x.z * (double)y.z;
            q += (double)x.w * (double)y.w;
        }
    }
    q = block_sum(q, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = q;
}

__global__ __launch_bounds__(THREADS) void k_sn_dw(const Table *__restrict__ T, unsigned check, GradTable G,
                                                   const double *__restrict__ partial, const float *__restrict__ u_saved,
                                                   const float *__restrict__ v_saved, const float *__restrict__ sigma, float *__restrict__ dw)
{
    __shared__ double red[WAVES];
    if (T->check != check || (int)blockIdx.x >= T->total_tiles) return;
    const TileOf o = tile_of(T);
    const Layer L = T->layer[o.l];
    const int first = T->first_tile[o.l], tiles = T->first_tile[o.l + 1] - first;
    double q = 0.0;
    for (int j = threadIdx.x; j < tiles; j += THREADS) q += partial[first + j];
    const float d = (float)block_sum(q, red), sg = sigma[o.l];
    const float *g = G.g[o.l] ? G.g[o.l] + o.at : nullptr;
    const float *us = u_saved + L.row_off, *vs = v_saved + L.col_off;
    float *dst = dw + L.elem_off + o.at;
    const bool vec = g && aligned16_dev(g), one_row = L.C % 4 == 0;
    for (int i = 4 * threadIdx.x; i < o.len; i += 4 * THREADS) {
        const int m = min(4, o.len - i), e = o.at + i;
        float4 x = {0.0f, 0.0f, 0.0f, 0.0f};
        if (g) x = load4(g + i, vec && m == 4, m);
        float4 y;
        if (one_row) {                          // (four values of one row: e is a multiple of 4)
            const int r = e / L.C, c = e - r * L.C;
            const float du = d * us[r];
            const float4 v4 = *reinterpret_cast<const float4 *>(vs + c);
            y.x = (x.x - du * v4.x) / sg;
            y.y = (x.y - du * v4.y) / sg;
            y.z = (x.z - du * v4.z) / sg;
            y.w = (x.w - du * v4.w) / sg;
        } else {
            float in[4] = {x.x, x.y, x.z, x.w}, out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < m; ++k) {
                const int r = (e + k) / L.C, c = (e + k) - r * L.C;
                out[k] = (in[k] - (d * us[r]) * vs[c]) / sg;
            }
            y.x = out[0];
            y.y = out[1];
            y.z = out[2];
            y.w = out[3];
        }
        store4(dst + i, m == 4, m, y);
    }
}

inline unsigned hash_of(const Table &T)
{
    const unsigned char *p = reinterpret_cast<const unsigned char *>(&T) + offsetof(Table, n_layers);
    unsigned h = 2166136261u;                   // FNV-1a over everything behind `check`
    for (size_t i = 0; i < sizeof(Table) - offsetof(Table, n_layers); ++i) h = (h ^ p[i]) * 16777619u;
    return h;
}

// The three regions of the workspace, all doubles: the parts of W^T u, the tiles' shares of d, s
struct Regions {
    size_t tu, partial, s, bytes;
};

inline Regions regions_of(const Table &T)
{
    Regions g;
    g.tu = 0;
    g.partial = ps::align_up((size_t)T.total_tu * sizeof(double), 256);
    g.s = g.partial + ps::align_up((size_t)T.total_tiles * sizeof(double), 256);
    g.bytes = g.s + ps::align_up((size_t)T.total_rows * sizeof(double), 256);
    return g;
}

inline const Table *table_of(const void *host)
{
    const Table *T = static_cast<const Table *>(host);
    if (!T || T->magic != MAGIC || T->n_layers < 1 || T->n_layers > MAX_LAYERS || T->check != hash_of(*T)) return nullptr;
    return T;
}

}  // namespace

extern "C" {

const char *ps_spectral_train_last_error(void) { return ps::last_error_ref().c_str(); }

size_t ps_spectral_table_bytes(void) { return sizeof(Table); }

int ps_spectral_plan(const void *const *weights, const void *const *us, const void *const *vs, const int *rows, const int *cols,
                     const int *interleave, const int *iterate, const float *eps, int n_layers, void *table, size_t table_bytes,
                     long long *elem_offsets, long long *row_offsets, long long *col_offsets)
{
    PS_REQUIRE(weights && us && vs && rows && cols && interleave && iterate && eps && table, "spectral_plan: null pointer");
    PS_REQUIRE(n_layers >= 1 && n_layers <= MAX_LAYERS, "spectral_plan: n_layers = %d, expected 1 .. %d", n_layers, MAX_LAYERS);
    PS_REQUIRE(table_bytes >= sizeof(Table), "spectral_plan: a table of %zu bytes, %zu needed", table_bytes, sizeof(Table));
    Table T;
    memset(&T, 0, sizeof(T));
    T.magic = MAGIC;
    T.n_layers = n_layers;
    long long parts = 0, rowgroups = 0, tiles = 0;
    for (int k = 0; k < n_layers; ++k) {
        const long long R = rows[k], C = cols[k];
        PS_REQUIRE(R >= 1 && C >= 1 && R * C < (1ll << 31), "spectral_plan: layer %d is %lld x %lld, expected R, C >= 1 and R C < 2^31", k,
                   R, C);
        PS_REQUIRE(weights[k] && us[k] && vs[k], "spectral_plan: null pointer (layer %d)", k);
        PS_REQUIRE(((uintptr_t)weights[k] & 3) == 0 && ((uintptr_t)us[k] & 3) == 0 && ((uintptr_t)vs[k] & 3) == 0,
                   "spectral_plan: layer %d is not aligned to 4 bytes", k);
        PS_REQUIRE(interleave[k] >= 1 && C % interleave[k] == 0, "spectral_plan: layer %d has interleave = %d, expected a divisor of C = %lld",
                   k, interleave[k], C);
        PS_REQUIRE(eps[k] > 0.0f, "spectral_plan: layer %d has eps = %g, expected > 0", k, (double)eps[k]);
        Layer &L = T.layer[k];
        L.W = static_cast<const float *>(weights[k]);
        L.u = static_cast<float *>(const_cast<void *>(us[k]));
        L.v = static_cast<float *>(const_cast<void *>(vs[k]));
        L.R = (int)R;
        L.C = (int)C;
        L.iterate = iterate[k] != 0;
        L.eps = eps[k];
        L.inter = interleave[k];
        L.parts = (int)((R + PART_ROWS - 1) / PART_ROWS);
        L.elem_off = T.total_elems;
        L.tu_off = T.total_tu;
        L.row_off = (int)T.total_rows;
        L.col_off = (int)T.total_cols;
        T.first_part[k] = (int)parts;
        T.first_rowgroup[k] = (int)rowgroups;
        T.first_tile[k] = (int)tiles;
        parts += L.parts;
        rowgroups += (R + WAVES - 1) / WAVES;
        tiles += (R * C + TILE - 1) / TILE;
        T.total_elems += (R * C + 3) / 4 * 4;
        T.total_tu += (long long)L.parts * C;
        T.total_rows += R;
        T.total_cols += (C + 3) / 4 * 4;
        PS_REQUIRE(T.total_elems < (1ll << 40) && T.total_rows < (1ll << 31) && T.total_cols < (1ll << 31) && parts < (1ll << 31)
                       && rowgroups < (1ll << 31) && tiles < (1ll << 31),
                   "spectral_plan: the table is too large at layer %d", k);
    }
    for (int k = n_layers; k <= MAX_LAYERS; ++k) {
        T.first_part[k] = (int)parts;
        T.first_rowgroup[k] = (int)rowgroups;
        T.first_tile[k] = (int)tiles;
    }
    T.total_parts = (int)parts;
    T.total_rowgroups = (int)rowgroups;
    T.total_tiles = (int)tiles;
    T.check = hash_of(T);
    memcpy(table, &T, sizeof(T));
    for (int k = 0; k <= n_layers; ++k) {
        const bool end = k == n_layers;
        if (elem_offsets) elem_offsets[k] = end ? T.total_elems : T.layer[k].elem_off;
        if (row_offsets) row_offsets[k] = end ? T.total_rows : T.layer[k].row_off;
        if (col_offsets) col_offsets[k] = end ? T.total_cols : T.layer[k].col_off;
    }
    return PS_OK;
}

size_t ps_spectral_workspace_bytes(const void *table)
{
    const Table *T = table_of(table);
    return T ? regions_of(*T).bytes : 0;
}

#define SPECTRAL_TABLE(what)                                                                                                          \
    const Table *T = table_of(table_host);                                                                                            \
    PS_REQUIRE(T, what ": table_host is not a table ps_spectral_plan filled");                                                        \
    PS_REQUIRE(table_device, what ": null pointer (table_device)");                                                                   \
    const Regions reg = regions_of(*T);                                                                                               \
    PS_REQUIRE(workspace, what ": null pointer (workspace)");                                                                         \
    PS_REQUIRE(workspace_bytes >= reg.bytes, what ": workspace of %zu bytes, %zu needed", workspace_bytes, reg.bytes);                \
    PS_REQUIRE(ps::aligned16(workspace), what ": the workspace must be aligned to 16 bytes");                                         \
    const Table *D = static_cast<const Table *>(table_device);                                                                        \
    hipStream_t st = (hipStream_t)stream;                                                                                             \
    char *ws = static_cast<char *>(workspace);                                                                                        \
    const dim3 block(THREADS)

int ps_spectral_forward_f32(const void *table_host, const void *table_device, float *w_sn, float *u_saved, float *v_saved, float *sigma,
                            void *workspace, size_t workspace_bytes, void *stream)
{
    SPECTRAL_TABLE("spectral_forward");
    PS_REQUIRE(w_sn && u_saved && v_saved && sigma, "spectral_forward: null pointer");
    PS_REQUIRE(ps::aligned16(w_sn) && ps::aligned16(v_saved), "spectral_forward: w_sn and v_saved must be aligned to 16 bytes");
    double *tu = reinterpret_cast<double *>(ws + reg.tu);
    double *s = reinterpret_cast<double *>(ws + reg.s);
    hipLaunchKernelGGL(k_sn_wtu, dim3(T->total_parts), block, 0, st, D, T->check, tu);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sn_v, dim3(T->n_layers), block, 0, st, D, T->check, tu, v_saved);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sn_wv, dim3(T->total_rowgroups), block, 0, st, D, T->check, (const float *)v_saved, s);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sn_u, dim3(T->n_layers), block, 0, st, D, T->check, (const double *)s, u_saved, sigma);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sn_div, dim3(T->total_tiles), block, 0, st, D, T->check, (const float *)sigma, w_sn);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_spectral_backward_f32(const void *table_host, const void *table_device, const void *const *grads, const float *w_sn,
                             const float *u_saved, const float *v_saved, const float *sigma, float *dw, void *workspace,
                             size_t workspace_bytes, void *stream)
{
    SPECTRAL_TABLE("spectral_backward");
    PS_REQUIRE(grads && w_sn && u_saved && v_saved && sigma && dw, "spectral_backward: null pointer");
    PS_REQUIRE(ps::aligned16(w_sn) && ps::aligned16(v_saved) && ps::aligned16(dw),
               "spectral_backward: w_sn, v_saved and dw must be aligned to 16 bytes");
    GradTable G;
    for (int k = 0; k < MAX_LAYERS; ++k) {
        G.g[k] = k < T->n_layers ? static_cast<const float *>(grads[k]) : nullptr;
        PS_REQUIRE(((uintptr_t)G.g[k] & 3) == 0, "spectral_backward: the gradient of layer %d is not aligned to 4 bytes", k);
    }
    double *partial = reinterpret_cast<double *>(ws + reg.partial);
    hipLaunchKernelGGL(k_sn_dot, dim3(T->total_tiles), block, 0, st, D, T->check, G, w_sn, partial);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sn_dw, dim3(T->total_tiles), block, 0, st, D, T->check, G, (const double *)partial, u_saved, v_saved, sigma, dw);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
