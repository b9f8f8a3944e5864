// vq_train.hip -- the training half of the VQ-VAE's quantiser for gfx950 (MI355X): the straight-through output and the commitment term,
// the per-code statistics, the EMA update of the codebook, and the backward pass (the reference's Quantize.forward in training mode,
// models/vqvae2/vqvae.py:41-74, which builds an (N,K) distance matrix, an (N,K) one-hot and two dense products against it).
//
// Behind the C ABI of include/pixelsynth_vq_train.h (libpixelsynth_vq_train.so, beside libpixelsynth_hip.so whose set of exports it
// leaves as it is; the codes are that library's ps_vq_nearest_f32).
//
//   k_stats_parts    sums = z^T (D x N) . onehot (N x K) on v_mfma_f32_16x16x4_f32 (lane l holds A[l&15][l>>4] and B[l>>4][l&15]): one
//                    wave per (part of the rows, 32 codes) keeps the 16 x 16 accumulator tiles of up to four channel tiles times two
//                    code tiles -- eight independent chains.  A is a 16-channel x 4-row slice of z as it lies; B is idx[n] == k ? 1 : 0,
//                    made in registers from one load of the four rows' codes.  Products with 0 and 1 are exact, so a sum is the fp32
//                    additions of its terms in ascending row.  A row past the part's end, a channel past D and a code tile past K load
//                    an address inside the buffers and are zeroed.  The next batch of steps' operands is loaded before the current one's MFMAs.
//                    The same lanes count their matches with integer adds.  Each part writes its tiles to the workspace.
//   k_stats_sum      adds the partial tables in ascending order of the part and writes sums (D,K) and counts (K).
//   k_quantize       z + (rows[idx] - z) and the fp64 partial sum of the squared residual per workgroup; k_diff_final adds the partials
//                    in ascending order.
//   k_update_cluster cluster_size, n and s (one workgroup); k_update_embed embed_avg and the new codebook.
//   k_backward       one gather pass.
// No float atomics, no integer ones either: every sum has one fixed order.
#include "ps_common.h"

#include "../../include/pixelsynth_vq_train.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int TILE = 16;                        // channels / codes of an MFMA tile
constexpr int KSTEP = 4;                        // rows per MFMA
constexpr int DT_MAX = 4;                       // channel tiles a wave keeps: D <= 64
constexpr int CT = 2;                           // code tiles a wave keeps
constexpr int DEPTH = 2;                        // steps whose operands are loaded together, one batch ahead of their MFMAs
constexpr int MAX_D = DT_MAX * TILE;
constexpr int MAX_N = 1 << 30, MAX_K = 1 << 20;
constexpr int Q_PER_THREAD = 64, Q_ELEMS = THREADS * Q_PER_THREAD;     // elements of k_quantize's workgroup

struct Plan {
    int Dp, Kp, dt, kt, wpp, part_rows, parts;
    long long qwgs;
    size_t psums, pcounts, qpart, s, bytes;     // byte offsets into the workspace, and its size
};

inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

inline bool sizes_ok(int N, int D, int K) { return N >= 1 && D >= 1 && K >= 1 && D <= MAX_D && N <= MAX_N && K <= MAX_K; }

// The split of the rows and the layout of the workspace: a function of the sizes alone
inline Plan make_plan(int N, int D, int K)
{
    Plan p;
    p.Dp = (int)ceil_div(D, TILE) * TILE;
    p.Kp = (int)ceil_div(K, TILE) * TILE;
    p.dt = p.Dp / TILE;
    p.kt = p.Kp / TILE;
    p.wpp = (int)ceil_div(p.kt, CT);            // waves per part
    const long long blocks = ceil_div(N, PS_VQ_TRAIN_PART_ROWS);
    p.part_rows = (int)(PS_VQ_TRAIN_PART_ROWS * ceil_div(blocks, PS_VQ_TRAIN_MAX_PARTS));
    p.parts = (int)ceil_div(N, p.part_rows);
    p.qwgs = ceil_div((long long)N * D, Q_ELEMS);
    p.psums = 0;
    p.pcounts = ps::align_up(p.psums + (size_t)p.parts * p.Dp * p.Kp * sizeof(float), 256);
    p.qpart = ps::align_up(p.pcounts + (size_t)p.parts * p.Kp * sizeof(int32_t), 256);
    p.s = ps::align_up(p.qpart + (size_t)p.qwgs * sizeof(double), 256);
    p.bytes = ps::align_up(p.s + (size_t)K * sizeof(float), 256);
    return p;
}

// The operands of DEPTH steps of one lane: its row's code and its row's value in each channel tile
template <int DT> struct Operands {
    float a[DEPTH][DT];
    int code[DEPTH];
    bool valid[DEPTH];
};

// One wave per (part, CT code tiles), the code range fastest: the waves of a workgroup read the same rows of z.  No LDS, no barrier:
// a wave without a task leaves.  DT: the channel tiles, ceil(D / 16).
template <int DT>
__global__ __launch_bounds__(THREADS) void k_stats_parts(const float *__restrict__ z, const int32_t *__restrict__ idx, int N, int D, int Dp,
                                                         int Kp, int kt, int wpp, int part_rows, int parts,
                                                         float *__restrict__ psums, int32_t *__restrict__ pcounts)
{
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (w >= (long long)parts * wpp) return;
    const int p = (int)(w / wpp), cr = (int)(w % wpp);
    const int kr = lane >> 4, col = lane & 15;
    const int n0 = p * part_rows, n1 = min(n0 + part_rows, N);         // (n0 < N: no empty part)
    const bool c_hi = cr * CT + 1 < kt;                                // (the second code tile may lie past the codes)
    const int k0 = cr * CT * TILE + col, k1 = k0 + TILE;
    int doff[DT];                                                      // this lane's channel in each tile; past D: channel 0, zeroed
    bool dok[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        dok[t] = t * TILE + col < D;
        doff[t] = dok[t] ? t * TILE + col : 0;
    }
    f32x4 acc[DT][CT];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[t][c] = f32x4{0, 0, 0, 0};
    int cnt0 = 0, cnt1 = 0;

    // The operands of the DEPTH steps from row `base`, without a branch: a row past the part's end loads row n0.  What is loaded is
    // zeroed where it is used, one batch later: a select beside the load would let the compiler put the load under a branch and wait
    // for it there.
    auto load = [&](int base, Operands<DT> &o) {
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            const int row = base + u * KSTEP + kr;
            const bool valid = row < n1;
            const int safe = valid ? row : n0;
            const int code = idx[safe];
            o.code[u] = code;
            o.valid[u] = valid;
            const float *zr = z + (size_t)safe * D;
#pragma unroll
            for (int t = 0; t < DT; ++t) o.a[u][t] = zr[doff[t]];
        }
    };

    // The MFMAs of one batch, ascending rows: each accumulator stays one chain.  A batch that lies past the part's end adds exact zeros.
    auto product = [&](const Operands<DT> &o) {
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            const bool m0 = o.valid[u] && o.code[u] == k0, m1 = o.valid[u] && c_hi && o.code[u] == k1;
            const float b0 = m0 ? 1.0f : 0.0f, b1 = m1 ? 1.0f : 0.0f;
            cnt0 += m0;
            cnt1 += m1;
#pragma unroll
            for (int t = 0; t < DT; ++t) {
                const float a = o.valid[u] && dok[t] ? o.a[u][t] : 0.0f;
                acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc[t][0], 0, 0, 0);
                acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc[t][1], 0, 0, 0);
            }
        }
    };

    // Two batches in turn, each loaded while the other's MFMAs run
    constexpr int BATCH = DEPTH * KSTEP;
    Operands<DT> even, odd;
    load(n0, even);
    for (int base = n0; base < n1; base += 2 * BATCH) {
        load(base + BATCH, odd);
        product(even);
        load(base + 2 * BATCH, even);
        product(odd);
    }
    // C/D: lane holds rows 4 (lane >> 4) + r (channels), column lane & 15 (codes)
    float *out = psums + (size_t)p * Dp * Kp;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = t * TILE + 4 * kr + r;
            out[(size_t)d * Kp + k0] = acc[t][0][r];
            if (c_hi) out[(size_t)d * Kp + k1] = acc[t][1][r];
        }
    }
    // the four row groups' counts of a code: lanes col, col + 16, col + 32, col + 48
    cnt0 += __shfl_xor(cnt0, 16, 64);
    cnt0 += __shfl_xor(cnt0, 32, 64);
    cnt1 += __shfl_xor(cnt1, 16, 64);
    cnt1 += __shfl_xor(cnt1, 32, 64);
    if (kr == 0) {
        pcounts[(size_t)p * Kp + k0] = cnt0;
        if (c_hi) pcounts[(size_t)p * Kp + k1] = cnt1;
    }
}

// sums[d][k] = part 0 + part 1 + ... in that order (threads 0 .. D K - 1, k fastest), counts[k] likewise (the K threads after them)
__global__ __launch_bounds__(THREADS) void k_stats_sum(const float *__restrict__ psums, const int32_t *__restrict__ pcounts, int parts, int D,
                                                       int K, int Dp, int Kp, float *__restrict__ sums, int32_t *__restrict__ counts)
{
    const long long e = (long long)blockIdx.x * THREADS + threadIdx.x, DK = (long long)D * K;
    if (e < DK) {
        const int d = (int)(e / K), k = (int)(e % K);
        const float *src = psums + (size_t)d * Kp + k;
        const size_t stride = (size_t)Dp * Kp;
        float s = src[0];
        for (int p = 1; p < parts; ++p) s += src[(size_t)p * stride];
        sums[e] = s;
    } else if (e < DK + K) {
        const int k = (int)(e - DK);
        int c = 0;
        for (int p = 0; p < parts; ++p) c += pcounts[(size_t)p * Kp + k];
        counts[k] = c;
    }
}

// Channel d of code k; a code outside the codebook is a row of zeros
__device__ __forceinline__ float code_value(const float *__restrict__ rows, int k, int d, int D, int K)
{
    return (unsigned)k < (unsigned)K ? rows[(size_t)k * D + d] : 0.0f;
}

// Workgroup g over elements g Q_ELEMS + j THREADS + t, j ascending; the thread's squares added in that order in fp64, then a fixed
// pairwise tree over the 256 threads
__global__ __launch_bounds__(THREADS) void k_quantize(const float *__restrict__ z, const int32_t *__restrict__ idx, const float *__restrict__ rows,
                                                      long long total, int D, int K, float *__restrict__ q, double *__restrict__ partial)
{
    __shared__ double sh[THREADS];
    const int t = threadIdx.x;
    const long long first = (long long)blockIdx.x * Q_ELEMS;
    long long nb = first / D;                                          // element `first + j THREADS` is (row nb, channel db): uniform
    int db = (int)(first - nb * D);
    const int step_n = THREADS / D, step_d = THREADS % D;
    double acc = 0.0;
    for (int j = 0; j < Q_PER_THREAD; ++j) {
        const long long i = first + (long long)j * THREADS + t;
        if (i < total) {
            const unsigned x = (unsigned)(db + t);
            const long long n = nb + x / (unsigned)D;
            const int d = (int)(x % (unsigned)D);
            const float zv = z[i];
            const float r = code_value(rows, idx[n], d, D, K) - zv;
            q[i] = zv + r;
            acc += (double)r * (double)r;
        }
        nb += step_n;
        db += step_d;
        if (db >= D) { db -= D; ++nb; }
    }
    sh[t] = acc;
    __syncthreads();
    for (int off = THREADS / 2; off > 0; off >>= 1) {
        if (t < off) sh[t] += sh[t + off];
        __syncthreads();
    }
    if (t == 0) partial[blockIdx.x] = sh[0];
}

__global__ void k_diff_final(const double *__restrict__ partial, long long count, double total, float *__restrict__ diff)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (long long g = 0; g < count; ++g) s += partial[g];
    diff[0] = (float)(s / total);
}

// One workgroup: the new cluster sizes, their fp64 sum in ascending k, and s[k] for k_update_embed
__global__ __launch_bounds__(THREADS) void k_update_cluster(const int32_t *__restrict__ counts, int K, float decay, float alpha, float eps,
                                                            float *__restrict__ cluster, float *__restrict__ s)
{
    __shared__ float sh_n;
    const int t = threadIdx.x;
    for (int k = t; k < K; k += THREADS) cluster[k] = decay * cluster[k] + alpha * (float)counts[k];
    __syncthreads();
    if (t == 0) {
        double n = 0.0;
        for (int k = 0; k < K; ++k) n += (double)cluster[k];
        sh_n = (float)n;
    }
    __syncthreads();
    const float n = sh_n, den = n + (float)K * eps;
    for (int k = t; k < K; k += THREADS) s[k] = (cluster[k] + eps) / den * n;
}

__global__ __launch_bounds__(THREADS) void k_update_embed(const float *__restrict__ sums, const float *__restrict__ s, int D, int K, float decay,
                                                          float alpha, float *__restrict__ avg, float *__restrict__ embed)
{
    const long long e = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= (long long)D * K) return;
    const float a = decay * avg[e] + alpha * sums[e];
    avg[e] = a;
    embed[e] = a / s[e % K];
}

__global__ __launch_bounds__(THREADS) void k_backward(const float *__restrict__ z, const int32_t *__restrict__ idx, const float *__restrict__ rows,
                                                      const float *__restrict__ gq, const float *__restrict__ gd, long long total, int D, int K,
                                                      float *__restrict__ gi)
{
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const float g = gq ? gq[i] : 0.0f;
    const double c = gd ? (double)gd[0] * 2.0 / (double)total : 0.0;
    if (c == 0.0) {                                                    // (no commitment term: grad_quantize as it is, bit for bit)
        gi[i] = g;
        return;
    }
    const long long first = (long long)blockIdx.x * THREADS, nb = first / D;          // (uniform: the 64-bit division once per wave)
    const unsigned x = (unsigned)(first - nb * D) + threadIdx.x;
    const long long n = nb + x / (unsigned)D;
    const int d = (int)(x % (unsigned)D);
    const float r = z[i] - code_value(rows, idx[n], d, D, K);
    gi[i] = g + (float)(c * (double)r);
}

}  // namespace

extern "C" {

const char *ps_vq_train_last_error(void) { return ps::last_error_ref().c_str(); }

size_t ps_vq_train_workspace_bytes(int N, int D, int K)
{
    if (!sizes_ok(N, D, K)) return 0;
    return make_plan(N, D, K).bytes;
}

#define VQ_TRAIN_SIZES(what)                                                                                                      \
    PS_REQUIRE(N >= 1 && D >= 1 && K >= 1, what ": N = %d, D = %d, K = %d, expected all >= 1", N, D, K);                          \
    PS_REQUIRE(D <= MAX_D, what ": D = %d, more than %d (the limit of ps_vq_nearest_f32)", D, MAX_D);                             \
    PS_REQUIRE(sizes_ok(N, D, K), what ": N = %d, K = %d: more than 2^30 vectors or 2^20 codes", N, K)

#define VQ_TRAIN_WORKSPACE(what, need)                                                                                            \
    PS_REQUIRE(workspace, what ": null pointer (workspace)");                                                                     \
    PS_REQUIRE(workspace_bytes >= (need), what ": workspace of %zu bytes, %zu needed", workspace_bytes, (size_t)(need));          \
    PS_REQUIRE((uintptr_t)workspace % 16 == 0, what ": the workspace must be aligned to 16 bytes")

int ps_vq_train_stats_f32(const float *z, const int32_t *idx, int N, int D, int K, int32_t *counts, float *sums, void *workspace,
                          size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(z && idx && counts && sums, "vq_train_stats: null pointer");
    VQ_TRAIN_SIZES("vq_train_stats");
    const Plan p = make_plan(N, D, K);
    VQ_TRAIN_WORKSPACE("vq_train_stats", p.bytes);
    hipStream_t st = (hipStream_t)stream;
    float *psums = (float *)((char *)workspace + p.psums);
    int32_t *pcounts = (int32_t *)((char *)workspace + p.pcounts);
    const long long waves = (long long)p.parts * p.wpp;
    const dim3 grid((unsigned)ceil_div(waves, WAVES));
#define VQ_TRAIN_STATS(DT) \
    hipLaunchKernelGGL(k_stats_parts<DT>, grid, dim3(THREADS), 0, st, z, idx, N, D, p.Dp, p.Kp, p.kt, p.wpp, p.part_rows, p.parts, psums, pcounts)
    switch (p.dt) {
    case 1: VQ_TRAIN_STATS(1); break;
    case 2: VQ_TRAIN_STATS(2); break;
    case 3: VQ_TRAIN_STATS(3); break;
    default: VQ_TRAIN_STATS(4); break;
    }
#undef VQ_TRAIN_STATS
    PS_LAUNCH_CHECK();
    const long long elems = (long long)D * K + K;
    hipLaunchKernelGGL(k_stats_sum, dim3((unsigned)ceil_div(elems, THREADS)), dim3(THREADS), 0, st, psums, pcounts, p.parts, D, K, p.Dp,
                       p.Kp, sums, counts);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_vq_train_quantize_f32(const float *z, const int32_t *idx, const float *rows, int N, int D, int K, float *quantize, float *diff,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(z && idx && rows && quantize && diff, "vq_train_quantize: null pointer");
    VQ_TRAIN_SIZES("vq_train_quantize");
    const Plan p = make_plan(N, D, K);
    VQ_TRAIN_WORKSPACE("vq_train_quantize", p.bytes);
    hipStream_t st = (hipStream_t)stream;
    double *partial = (double *)((char *)workspace + p.qpart);
    const long long total = (long long)N * D;
    hipLaunchKernelGGL(k_quantize, dim3((unsigned)p.qwgs), dim3(THREADS), 0, st, z, idx, rows, total, D, K, quantize, partial);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_diff_final, dim3(1), dim3(64), 0, st, partial, p.qwgs, (double)total, diff);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_vq_train_update_f32(const int32_t *counts, const float *sums, int D, int K, float decay, float alpha, float eps,
                           float *cluster_size, float *embed_avg, float *embed_out, void *workspace, size_t workspace_bytes,
                           void *stream)
{
    const int N = 1;
    PS_REQUIRE(counts && sums && cluster_size && embed_avg && embed_out, "vq_train_update: null pointer");
    VQ_TRAIN_SIZES("vq_train_update");
    PS_REQUIRE(embed_out != embed_avg && embed_out != sums, "vq_train_update: embed_out cannot be embed_avg or sums");
    const Plan p = make_plan(N, D, K);
    VQ_TRAIN_WORKSPACE("vq_train_update", p.bytes);
    hipStream_t st = (hipStream_t)stream;
    // (laid out as for N = 1: the update does not know N, and a workspace sized for any N holds that of N = 1)
    float *s = (float *)((char *)workspace + p.s);
    hipLaunchKernelGGL(k_update_cluster, dim3(1), dim3(THREADS), 0, st, counts, K, decay, alpha, eps, cluster_size, s);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_update_embed, dim3((unsigned)ceil_div((long long)D * K, THREADS)), dim3(THREADS), 0, st, sums, s, D, K, decay, alpha,
                       embed_avg, embed_out);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_vq_train_backward_f32(const float *z, const int32_t *idx, const float *rows, const float *grad_quantize, const float *grad_diff,
                             int N, int D, int K, float *grad_input, void *stream)
{
    PS_REQUIRE(grad_input && (grad_quantize || grad_diff), "vq_train_backward: null pointer (grad_input, or both gradients)");
    PS_REQUIRE(!grad_diff || (z && idx && rows), "vq_train_backward: null pointer (grad_diff needs z, idx and rows)");
    VQ_TRAIN_SIZES("vq_train_backward");
    const long long total = (long long)N * D;
    hipLaunchKernelGGL(k_backward, dim3((unsigned)ceil_div(total, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, z, idx, rows, grad_quantize,
                       grad_diff, total, D, K, grad_input);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
