// rank.hip -- scoring and ranking the best-of-N candidates of a view on the device, for gfx950 (MI355X): what get_best_sample does per
// candidate on the host (reference: models/z_buffermodel.py:254-276) around its two scorer networks.
//
// Behind the C ABI of include/pixelsynth_rank.h (libpixelsynth_rank.so, a library of its own beside libpixelsynth_hip.so).  Four passes,
// none with an atomic, each with a fixed order of summation:
//   k_rank_input   candidates -> the classifier's input.  One workgroup per (candidate, band of <= 16 output rows): the horizontal pass
//                  of Pillow's resample reads the input rows the band needs (lanes along the interleaved (x, c) axis: coalesced but for
//                  the resample's stride), quantises every tap as the host does and leaves its uint8 result in LDS; the vertical pass
//                  runs with consecutive lanes along x, so that the planar stores coalesce, and looks the normalised value up in the
//                  host's 3 x 256 table.  Table-driven: the bounds and 22-bit weights are Pillow's, made by the host.
//   k_rank_entropy one wave per row of logits: maximum, sum of exp, sum of p log p; per-lane strided partial results, one butterfly each.
//   k_rank_hinge   one wave per candidate: the hinge term of every element of its two patch maps, summed in fp64.
//   k_rank_select  one workgroup: both lists in LDS, every element's rank by counting, the packed (total, index) maximum
//                  (rank_select.h: libpixelsynth_rank_groups.so runs the same code once per view of a batch).
// The unit is built with -ffp-contract=off: the quantisation's three fp32 operations stay three.
#include "ps_common.h"

#include "../../include/pixelsynth_rank.h"
#include "rank_select.h"

namespace {

constexpr int RANK_THREADS = 256;
static_assert(RANK_THREADS == ps_rank::SELECT_THREADS, "k_rank_select is one workgroup of select_group");
constexpr int BAND_ROWS = 16;                        // output rows of a workgroup of k_rank_input, fewer where LDS asks for it
constexpr size_t BAND_LDS_BYTES = 48 * 1024;         // at most, for the horizontal pass's rows
constexpr int PRECISION_BITS = 32 - 8 - 2;           // Pillow's (src/libImaging/Resample.c)

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// ((x * .5 + .5) * 255).astype(uint8) of an fp32 x.  Outside [-1,1] (see the header): clamped into int32, NaN -> the lower clamp -> 0.
__device__ __forceinline__ uint32_t quantise(float x)
{
    float v = __fmul_rn(__fadd_rn(__fmul_rn(x, 0.5f), 0.5f), 255.0f);
    v = fminf(fmaxf(v, -2147483648.0f), 2147483520.0f);
    return (uint32_t)(int)v & 0xffu;
}

// clip8 of Pillow: (ss >> PRECISION_BITS) into 0..255.  The sum is carried modulo 2^32 (it cannot wrap with Pillow's tables)
__device__ __forceinline__ uint32_t clip8(uint32_t ss) { return (uint32_t)clampi((int)ss >> PRECISION_BITS, 0, 255); }

__global__ __launch_bounds__(RANK_THREADS) void k_rank_input(const float *__restrict__ imgs, int S, int T,
                                                             const int32_t *__restrict__ bounds, const int32_t *__restrict__ coeffs,
                                                             int ksize, const float *__restrict__ norm, float *__restrict__ out,
                                                             uint8_t *__restrict__ bytes, int band, int rows_max, int pitch)
{
    extern __shared__ uint8_t s_h[];                 // (rows, pitch): the horizontal pass of input rows r0 .. r0 + rows - 1
    const int tid = threadIdx.x, n = blockIdx.y;
    const int y0 = blockIdx.x * band, y1 = min(y0 + band, T), W3 = 3 * T;
    const float *img = imgs + (size_t)n * 3 * S * S;
    // the band's input rows: the first tap of its first output row to the last tap of its last one (the bounds rise with the index)
    const int r0 = clampi(bounds[2 * y0], 0, S);
    const int rows = min(clampi(bounds[2 * (y1 - 1)] + bounds[2 * (y1 - 1) + 1], r0, S) - r0, rows_max);

    for (int idx = tid; idx < rows * W3; idx += RANK_THREADS) {
        const int r = idx / W3, j = idx - r * W3, x = j / 3, c = j - 3 * x;
        const int xmin = clampi(bounds[2 * x], 0, S), cnt = clampi(bounds[2 * x + 1], 0, min(ksize, S - xmin));
        const float *p = img + ((size_t)(r0 + r) * S + xmin) * 3 + c;
        const int32_t *k = coeffs + (size_t)x * ksize;
        uint32_t ss = 1u << (PRECISION_BITS - 1);
        for (int t = 0; t < cnt; ++t) ss += quantise(p[3 * t]) * (uint32_t)k[t];
        s_h[r * pitch + j] = (uint8_t)clip8(ss);
    }
    __syncthreads();

    for (int idx = tid; idx < (y1 - y0) * W3; idx += RANK_THREADS) {
        const int yy = idx / W3, rest = idx - yy * W3, c = rest / T, x = rest - c * T, y = y0 + yy;
        const int ymin = clampi(bounds[2 * y], 0, S), cnt = clampi(bounds[2 * y + 1], 0, min(ksize, S - ymin));
        const int32_t *k = coeffs + (size_t)y * ksize;
        uint32_t ss = 1u << (PRECISION_BITS - 1);
        for (int t = 0; t < cnt; ++t) {
            const int r = ymin + t - r0;
            if ((unsigned)r < (unsigned)rows) ss += (uint32_t)s_h[r * pitch + 3 * x + c] * (uint32_t)k[t];   // (always, with Pillow's tables)
        }
        const uint32_t u = clip8(ss);
        out[(((size_t)n * 3 + c) * T + y) * T + x] = norm[c * 256 + u];
        if (bytes) bytes[(((size_t)n * T + y) * T + x) * 3 + c] = (uint8_t)u;
    }
}

// the same value in every lane: fp32 addition and maximum are commutative, the butterfly pairs the same operands in every lane
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(64) void k_rank_entropy(const float *__restrict__ logits, int C, float *__restrict__ entropy)
{
    const int lane = threadIdx.x;
    const float *row = logits + (size_t)blockIdx.x * C;
    float m = -INFINITY;
    for (int i = lane; i < C; i += 64) m = fmaxf(m, row[i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    float s = 0.0f;
    for (int i = lane; i < C; i += 64) s += expf(row[i] - m);
    s = wave_sum(s);
    float h = 0.0f;
    for (int i = lane; i < C; i += 64) {
        const float p = expf(row[i] - m) / s;
        h += p * logf(p);                            // p == 0: 0 * -inf = NaN, kept (the header)
    }
    h = wave_sum(h);
    if (lane == 0) entropy[blockIdx.x] = -h;
}

// -sum min(-x - 1, 0) over a map, in every lane; a NaN stays one (torch.min hands it on)
__device__ __forceinline__ double hinge_sum(const float *__restrict__ map, int len, int lane)
{
    double acc = 0.0;
    for (int i = lane; i < len; i += 64) {
        const float t = __fsub_rn(-map[i], 1.0f);
        acc -= (double)(t > 0.0f ? 0.0f : t);
    }
    return wave_sum(acc);
}

__global__ __launch_bounds__(64) void k_rank_hinge(const float *__restrict__ map0, int len0, const float *__restrict__ map1, int len1,
                                                   float *__restrict__ d_fake)
{
    const int lane = threadIdx.x, n = blockIdx.x;
    const double m0 = hinge_sum(map0 + (size_t)n * len0, len0, lane) / (double)len0;
    const double m1 = hinge_sum(map1 + (size_t)n * len1, len1, lane) / (double)len1;
    if (lane == 0) d_fake[n] = (float)(0.5 * (m0 + m1));
}

// the rank rule itself is rank_select.h's, shared with rank_groups.hip (one workgroup per group of candidates there, one group here)
__global__ __launch_bounds__(RANK_THREADS) void k_rank_select(const float *__restrict__ disc, const float *__restrict__ entr, int n,
                                                              int32_t *__restrict__ best, int32_t *__restrict__ disc_rank,
                                                              int32_t *__restrict__ entr_rank)
{
    ps_rank::select_group(disc, entr, n, 1, best, disc_rank, entr_rank);
}

}  // namespace

extern "C" {

const char *ps_rank_last_error(void) { return ps::last_error_ref().c_str(); }

int ps_rank_classifier_input(const float *imgs, int N, int S, int T, const int32_t *bounds, const int32_t *coeffs, int ksize,
                             const float *norm, float *out, uint8_t *bytes, void *stream)
{
    PS_REQUIRE(imgs && bounds && coeffs && norm && out, "rank_classifier_input: null pointer");
    PS_REQUIRE(N > 0 && N <= 65535, "rank_classifier_input: N = %d, expected 1 .. 65535", N);
    PS_REQUIRE(S >= 1 && S <= PS_RANK_MAX_SIDE && T >= 1 && T <= PS_RANK_MAX_SIDE,
               "rank_classifier_input: S = %d, T = %d, expected 1 .. %d", S, T, PS_RANK_MAX_SIDE);
    PS_REQUIRE(ksize >= 1, "rank_classifier_input: ksize = %d, expected >= 1", ksize);
    // The input rows of a band of `band` output rows: the first tap of a row lies above center - support - 0.5, the last one below
    // center + support + 0.5, the centers are scale apart.  The band shrinks until its rows fit into LDS (one row always does).
    const double scale = (double)S / T, support = scale > 1.0 ? scale : 1.0;
    const int pitch = (3 * T + 3) & ~3;
    int band = BAND_ROWS < T ? BAND_ROWS : T, rows_max;
    for (;; --band) {
        const int need = (int)((band - 1) * scale + 2.0 * support) + 3;
        rows_max = need < S ? need : S;
        if ((size_t)rows_max * pitch <= BAND_LDS_BYTES || band == 1) break;
    }
    PS_REQUIRE((size_t)rows_max * pitch <= BAND_LDS_BYTES, "rank_classifier_input: S = %d, T = %d does not fit into LDS", S, T);
    hipLaunchKernelGGL(k_rank_input, dim3((T + band - 1) / band, N), dim3(RANK_THREADS), (size_t)rows_max * pitch, (hipStream_t)stream,
                       imgs, S, T, bounds, coeffs, ksize, norm, out, bytes, band, rows_max, pitch);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_rank_entropy(const float *logits, int N, int n_classes, float *entropy, void *stream)
{
    PS_REQUIRE(logits && entropy, "rank_entropy: null pointer");
    PS_REQUIRE(N > 0 && n_classes > 0, "rank_entropy: N = %d, n_classes = %d, expected > 0", N, n_classes);
    hipLaunchKernelGGL(k_rank_entropy, dim3(N), dim3(64), 0, (hipStream_t)stream, logits, n_classes, entropy);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_rank_hinge_fake(const float *map0, int len0, const float *map1, int len1, int N, float *d_fake, void *stream)
{
    PS_REQUIRE(map0 && map1 && d_fake, "rank_hinge_fake: null pointer");
    PS_REQUIRE(N > 0 && len0 > 0 && len1 > 0, "rank_hinge_fake: N = %d, len0 = %d, len1 = %d, expected > 0", N, len0, len1);
    hipLaunchKernelGGL(k_rank_hinge, dim3(N), dim3(64), 0, (hipStream_t)stream, map0, len0, map1, len1, d_fake);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_rank_select(const float *disc, const float *entr, int n, int32_t *best, int32_t *disc_rank, int32_t *entr_rank, void *stream)
{
    PS_REQUIRE(disc && entr && best, "rank_select: null pointer");
    PS_REQUIRE(n >= 1 && n <= PS_RANK_MAX_N, "rank_select: n = %d, expected 1 .. %d", n, PS_RANK_MAX_N);
    hipLaunchKernelGGL(k_rank_select, dim3(1), dim3(RANK_THREADS), 0, (hipStream_t)stream, disc, entr, n, best, disc_rank, entr_rank);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
