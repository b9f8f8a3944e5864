// conv_bwd.hip -- the backward pass of the split-fp16 3 x 3 convolution (csrc/conv_f16x3.hip) for gfx950 (MI355X): the gradient with
// respect to the weight on the fp16 matrix pipe, the gradient with respect to the bias, and the power-of-two scaling of grad_y that
// the operand split needs for gradients (include/pixelsynth_conv_bwd.h says why).  The gradient with respect to the input is the
// forward kernel itself, run by the caller on the scaled grad_y with the flipped, transposed weight.
//
// Behind the C ABI of include/pixelsynth_conv_bwd.h (libpixelsynth_conv_bwd.so, beside libpixelsynth_hip.so whose set of exports it
// leaves as it is).
//
//   grad_W[o,t,c] = sum_n g[n,o] * xpad[n + off(t), c],  n = (b,y,x) over the B*H*W pixels
//
// is a GEMM with M = Co, N = 9 Ci whose reduction runs over the pixels -- and both operands arrive channel-minor, the wrong way round
// for an MFMA whose lanes hold eight consecutive values of the reduction index.  The transpose is the LDS read:
//   k_grad_weight_parts   one workgroup = 4 waves = 64 output channels x 64 input channels x 9 taps of one part (a run of consecutive
//                         pixel tiles of 4 rows x 16 pixels); wave w owns output channels 32 (w & 1) .., input channels 32 (w >> 1) ..:
//                         nine 32 x 32 accumulator tiles (144 registers; two workgroups share a compute unit).  Per tile the 64 pixels
//                         of g and the 6 x 18 patch of x are split (hi = fp16(v), lo = fp16(v - hi), exactly the forward's stash())
//                         and written to LDS PIXEL-major, one row [hi: 64 channels | lo: 64 channels | 64 bytes of padding] = 320 bytes
//                         per pixel, channel-minor as they lie in memory.  ds_read_b64_tr_b16 then hands every lane four consecutive
//                         PIXELS of its channel: two of them are one operand of v_mfma_f32_32x32x16_f16 (lanes 0-31: pixels 0-7 of the
//                         tile row, lanes 32-63: pixels 8-15).  A tap's (ky, kx) shift is a whole number of 320-byte rows, so every
//                         read stays 8-byte aligned and all of them are one per-lane base plus an immediate; the four rows a 16-lane
//                         group reads are 320 bytes apart = 64 bytes apart in the 256-byte bank row: conflict-free.  Patch pixels
//                         outside the frame are written as zeros.  (A tile fetched into registers while the one before it
//                         multiplies costs 44 registers beside the 144 accumulators and the fragments the compiler keeps across
//                         rows, and spills; the other workgroup of the compute unit multiplies while this one fetches.)
//   k_grad_weight_sum     adds the partial tiles in ascending order of the part, times 1 / s, and writes (Co,3,3,Ci).
//   k_prep_partial / k_prep_finish   max|g| and the per-channel sums of g in one pass (fixed trees), then s and 1 / s.
//   k_scale               g * s into a copy; y *= 1 / s in place.
// No atomics anywhere: every sum has one fixed order, and the split into parts depends on the sizes alone.
#include "ps_common.h"

#include <cfloat>
#include <cmath>

#include "../../include/pixelsynth_conv_bwd.h"

namespace {

typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NT = 256;                       // threads of every kernel here
constexpr int TR = 4, TW = 16;                // a pixel tile: rows x pixels (one MFMA step per row)
constexpr int PR = TR + 2, PW = TW + 2;       // the patch of x behind it
constexpr int CB = 64;                        // channels of either operand per workgroup
constexpr int ROW = 320;                      // bytes per pixel in LDS: hi (128) | lo (128) | padding (64)
constexpr int LO = 128;                       // the lo half of a row
constexpr int G_BYTES = TR * TW * ROW;        // 20 480
constexpr int X_BYTES = PR * PW * ROW;        // 34 560
constexpr int NG = TR * TW * (CB / 4) / NT;   // float4 loads of g per thread and tile: 4
constexpr int NX = (PR * PW * (CB / 4) + NT - 1) / NT;   // of x: 7 (the last one partly)
constexpr int TARGET_WGS = 512;               // two workgroups on each of 256 compute units
constexpr int MIN_CHUNK = 8;                  // tiles a part has at least (but for the last): fewer are not worth a workgroup
constexpr int PREP_BLOCKS = 256;              // pixel ranges of the pass over g, at most
constexpr int PREP_MIN_PIXELS = 64;           // pixels of a range at least (but for the last): chains of four sums and a tree inside, chains across
constexpr long long MAX_PIXELS = 1LL << 30;

static_assert(G_BYTES + X_BYTES <= 64 * 1024, "static LDS");
static_assert(NG * NT == TR * TW * (CB / 4), "g: whole sweeps");

inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

struct Plan {
    int ntiles, blocks, chunk, parts;        // pixel tiles, 64 x 64 channel blocks, tiles per part, parts
    int npix, pchunk, nprep, ncb;            // the pass over g: pixels, pixels per range, ranges, 64-channel blocks of Co
    size_t amax, bytes;                      // byte offset of the ranges' maxima (their sums lie at 0), size of the workspace
};

inline bool sizes_ok(int B, int H, int W, int Ci, int Co)
{
    return B >= 1 && H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0 && Ci >= CB && Co >= CB && Ci % CB == 0 && Co % CB == 0
           && (long long)H * W * (Ci > Co ? Ci : Co) < (1LL << 31) && (long long)B * H * W <= MAX_PIXELS && Ci <= (1 << 16) && Co <= (1 << 16)
           && (long long)Ci * Co <= (1LL << 24);
}

// The split of the reduction and the layout of the workspace: a function of the sizes alone
inline Plan make_plan(int B, int H, int W, int Ci, int Co)
{
    Plan p;
    p.ntiles = B * (H / TR) * (W / TW);
    p.blocks = (Co / CB) * (Ci / CB);
    int want = ceil_div(TARGET_WGS, p.blocks);
    if (want > PS_CONV_BWD_MAX_PARTS) want = PS_CONV_BWD_MAX_PARTS;
    p.chunk = ceil_div(p.ntiles, want);
    if (p.chunk < MIN_CHUNK) p.chunk = MIN_CHUNK;
    p.parts = ceil_div(p.ntiles, p.chunk);      // (no empty part)
    p.npix = B * H * W;
    p.pchunk = ceil_div(p.npix, PREP_BLOCKS);
    if (p.pchunk < PREP_MIN_PIXELS) p.pchunk = PREP_MIN_PIXELS;
    p.nprep = ceil_div(p.npix, p.pchunk);
    p.ncb = Co / CB;
    p.amax = ps::align_up((size_t)p.nprep * Co * sizeof(float), 256);
    const size_t prep = ps::align_up(p.amax + (size_t)p.nprep * p.ncb * sizeof(float), 256);
    const size_t gw = ps::align_up((size_t)p.parts * 9 * Co * Ci * sizeof(float), 256);
    p.bytes = prep > gw ? prep : gw;
    return p;
}

// ---- the pass over g ---------------------------------------------------------------------------------------------------------------------
// grid (ranges, Co / 64): thread t sums channels 64 blockIdx.y + 4 (t & 15) .. + 3 over the pixels p0 + (t >> 4), + 16, ... of its range
// -- sixteen interleaved chains per channel, joined by a fixed tree: chain i with chain i + 8, then + 4, + 2, + 1
__global__ __launch_bounds__(NT) void k_prep_partial(const float *__restrict__ g, int npix, int pchunk, int Co, float *__restrict__ sums,
                                                     float *__restrict__ amax)
{
    __shared__ f32x4 sh_s[NT];
    __shared__ float sh_m[NT];
    const int t = threadIdx.x, o = blockIdx.y * CB + 4 * (t & 15);
    const int p0 = blockIdx.x * pchunk, p1 = min(p0 + pchunk, npix);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    float m = 0.0f;
    bool bad = false;
    for (int p = p0 + (t >> 4); p < p1; p += 16) {
        const f32x4 v = *(const f32x4 *)(g + (size_t)p * Co + o);
        s += v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = __builtin_fabsf(v[j]);
            bad |= !(a <= FLT_MAX);
            m = a > m ? a : m;
        }
    }
    sh_s[t] = s;
    sh_m[t] = bad ? INFINITY : m;
    __syncthreads();
    for (int off = NT / 2; off >= 16; off >>= 1) {
        if (t < off) sh_s[t] += sh_s[t + off];
        __syncthreads();
    }
    if (t < 16) *(f32x4 *)(sums + (size_t)blockIdx.x * Co + o) = sh_s[t];
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (t < off) sh_m[t] = sh_m[t] > sh_m[t + off] ? sh_m[t] : sh_m[t + off];
        __syncthreads();
    }
    if (t == 0) amax[blockIdx.x * gridDim.y + blockIdx.y] = sh_m[0];
}

// s = 2^(15 - e), max = f * 2^e with f in [0.5, 1); the exponent held in [-126, 126]; 1 for a maximum of 0 or one that is not finite
__device__ __forceinline__ void scale_of(float m, float *scale2)
{
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

// grid (Co / 64): the ranges' sums in four interleaved chains, joined (0 + 1) + (2 + 3); every workgroup finds the maximum, the first writes s
__global__ __launch_bounds__(NT) void k_prep_finish(const float *__restrict__ sums, const float *__restrict__ amax, int nprep, int ncb, int Co,
                                                    float *__restrict__ grad_bias, float *__restrict__ scale2)
{
    __shared__ float sh_s[NT], sh_m[NT];
    const int t = threadIdx.x, o = blockIdx.x * CB + (t & 63);
    float s = 0.0f, m = 0.0f;
    for (int r = t >> 6; r < nprep; r += 4) s += sums[(size_t)r * Co + o];
    for (int i = t; i < nprep * ncb; i += NT) m = amax[i] > m ? amax[i] : m;
    sh_s[t] = s;
    sh_m[t] = m;
    __syncthreads();
    if (t < 64 && grad_bias) grad_bias[o] = (sh_s[t] + sh_s[t + 64]) + (sh_s[t + 128] + sh_s[t + 192]);
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (t < off) sh_m[t] = sh_m[t] > sh_m[t + off] ? sh_m[t] : sh_m[t + off];
        __syncthreads();
    }
    if (t == 0 && blockIdx.x == 0) scale_of(sh_m[0], scale2);
}

__global__ __launch_bounds__(NT) void k_scale(const f32x4 *in, size_t n4, const float *__restrict__ scale2, int which,
                                              f32x4 *out)   // (out may be in)
{
    const float f = scale2[which];
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (size_t)gridDim.x * NT) out[i] = in[i] * f;
}

inline unsigned stream_grid(size_t n4)
{
    const size_t want = (n4 + NT - 1) / NT;
    return (unsigned)(want < (1u << 16) ? (want ? want : 1) : (1u << 16));
}

// ---- grad_weight ---------------------------------------------------------------------------------------------------------------------------
struct GwArgs {
    const float *x, *g;     // (B,H,W,Ci), (B,H,W,Co) scaled
    float *part;            // (parts, Co, 9, Ci)
    int *overflow;
    int H, W, Ci, Co, tiles_x, tiles_per_frame, ntiles, chunk, ncib;
};

typedef __fp16 tr_h4 __attribute__((__vector_size__(4 * sizeof(__fp16))));   // the builtin's own type
typedef __attribute__((address_space(3))) tr_h4 lds_h4;

// eight consecutive pixels of this lane's channel: the two transposed reads of rows .. + 3 and + 4 .. + 7 (compile-time offsets)
__device__ __forceinline__ h8 tr8(const char *p)
{
    const h4 a = __builtin_bit_cast(h4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4 *)p));
    const h4 b = __builtin_bit_cast(h4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4 *)(p + 4 * ROW)));
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// grid (parts, (Co / 64) (Ci / 64)).  Two workgroups per compute unit: 256 registers a lane.
__global__ __launch_bounds__(NT, 2) void k_grad_weight_parts(GwArgs a)
{
    __shared__ __attribute__((aligned(16))) char lds[G_BYTES + X_BYTES];
    char *const lg = lds, *const lx = lds + G_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, W = a.W, Ci = a.Ci, Co = a.Co;
    const int co0 = ((int)blockIdx.y / a.ncib) * CB, ci0 = ((int)blockIdx.y % a.ncib) * CB;
    const int t0 = blockIdx.x * a.chunk, t1 = min(t0 + a.chunk, a.ntiles);

    // ---- staging role: channels 4 c4 .. 4 c4 + 3 of the block, pixels (tid >> 4) + 16 i of the tile / of the patch
    const int c4 = tid & 15, s0 = tid >> 4;
    f32x4 rg[NG], rx[NX];
    int over = 0;
    auto fetch = [&](int tile) {
        const int b = tile / a.tiles_per_frame, tf = tile - b * a.tiles_per_frame;
        const int y0 = (tf / a.tiles_x) * TR, x0 = (tf % a.tiles_x) * TW;
        // (offsets inside a frame fit 32 bits: H*W*max(Ci,Co) < 2^31)
        const float *gb = a.g + (size_t)b * H * W * Co + co0 + 4 * c4;
        const float *xb = a.x + (size_t)b * H * W * Ci + ci0 + 4 * c4;
        const int gbase = (y0 * W + x0) * Co, xbase = (y0 * W + x0) * Ci;
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            const int s = s0 + 16 * i, r = s >> 4, px = s & 15;
            rg[i] = *(const f32x4 *)(gb + (gbase + (r * W + px) * Co));
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int s = s0 + 16 * i, pr = s / PW, pc = s - pr * PW, iy = y0 + pr - 1, ix = x0 + pc - 1;
            const bool ok = s < PR * PW && iy >= 0 && iy < H && ix >= 0 && ix < W;
            rx[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (ok) rx[i] = *(const f32x4 *)(xb + (xbase + ((pr - 1) * W + pc - 1) * Ci));
        }
    };
    auto split_to = [&](char *dst, f32x4 v) {     // the forward's stash(): hi = fp16(v), lo = fp16(v - hi)
        h4 hi, lo;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            hi[j] = (_Float16)v[j];
            lo[j] = (_Float16)(v[j] - (float)hi[j]);
        }
        *(h4 *)dst = hi;
        *(h4 *)(dst + LO) = lo;
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < NG; ++i) split_to(lg + (s0 + 16 * i) * ROW + 8 * c4, rg[i]);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int s = s0 + 16 * i;
            if (s >= PR * PW) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) over |= !(__builtin_fabsf(rx[i][j]) <= 65000.f);
            split_to(lx + s * ROW + 8 * c4, rx[i]);
        }
    };

    // ---- MFMA role.  A = g: A[m][k], m = output channel, k = pixel; B = x: B[k][n], n = input channel; both: lane = (m or n) + 32 (k / 8),
    // element k % 8.  The transposed read works per group of 16 lanes on a block of 4 rows (pixels) x 16 columns (channels): lane 4 q + p
    // of the group gives the address of row q, columns 4 p .. 4 p + 3, and receives column (lane & 15) of the four rows.
    const int it = wave & 1, jt = wave >> 1, kb = lane >> 5, gi = (lane >> 4) & 1, q = (lane >> 2) & 3, p = lane & 3;
    const char *const ga = lg + (kb * 8 + q) * ROW + (32 * it + 16 * gi + 4 * p) * 2;
    const char *const xa = lx + (kb * 8 + q) * ROW + (32 * jt + 16 * gi + 4 * p) * 2;
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int tile = t0; tile < t1; ++tile) {
        fetch(tile);
        __syncthreads();            // the previous tile's reads are done
        stash();
        __syncthreads();
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            const h8 ah = tr8(ga + r * TW * ROW), al = tr8(ga + r * TW * ROW + LO);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const char *xp = xa + ((r + t / 3) * PW + t % 3) * ROW;
                const h8 bh = tr8(xp), bl = tr8(xp + LO);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[t], 0, 0, 0);
            }
        }
    }
    // D[row][col]: col = lane & 31 = input channel, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) = output channel
    float *out = a.part + ((size_t)blockIdx.x * Co + co0 + 32 * it) * 9 * Ci + ci0 + 32 * jt + (lane & 31);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * kb;
            out[((size_t)row * 9 + t) * Ci] = acc[t][r];
        }
    if (over) *a.overflow = 1;
}

// grad_W = (part 0 + part 1 + ...) / s in that order; thread e = four consecutive elements of (Co,3,3,Ci)
__global__ __launch_bounds__(NT) void k_grad_weight_sum(const f32x4 *__restrict__ part, int parts, size_t n4, const float *__restrict__ scale2,
                                                        f32x4 *__restrict__ gw)
{
    const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e >= n4) return;
    f32x4 s = part[e];
    for (int p = 1; p < parts; ++p) s += part[(size_t)p * n4 + e];
    gw[e] = s * scale2[1];
}

}  // namespace

extern "C" {

const char *ps_conv_bwd_last_error(void) { return ps::last_error_ref().c_str(); }

size_t ps_conv3x3_bwd_workspace_bytes(int B, int H, int W, int Ci, int Co)
{
    if (!sizes_ok(B, H, W, Ci, Co)) return 0;
    return make_plan(B, H, W, Ci, Co).bytes;
}

int ps_conv3x3_bwd_parts(int B, int H, int W, int Ci, int Co)
{
    if (!sizes_ok(B, H, W, Ci, Co)) return 0;
    return make_plan(B, H, W, Ci, Co).parts;
}

int ps_conv3x3_bwd_prepare_f32(const float *g, int B, int H, int W, int Co, float *g_scaled, float *scale2, float *grad_bias,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(g && g_scaled && scale2 && workspace, "conv3x3_bwd_prepare: null pointer");
    PS_REQUIRE(g != g_scaled, "conv3x3_bwd_prepare: g_scaled cannot be g");
    PS_REQUIRE(sizes_ok(B, H, W, CB, Co), "conv3x3_bwd_prepare: B = %d, H = %d, W = %d, Co = %d: H and W multiples of 16, Co a multiple of 64, "
               "H*W*Co < 2^31 and B*H*W <= 2^30 required", B, H, W, Co);
    const Plan p = make_plan(B, H, W, CB, Co);
    PS_REQUIRE(workspace_bytes >= ps::align_up(p.amax + (size_t)p.nprep * p.ncb * sizeof(float), 256),
               "conv3x3_bwd_prepare: workspace of %zu bytes, too small", workspace_bytes);
    PS_REQUIRE((uintptr_t)workspace % 16 == 0 && (uintptr_t)g % 16 == 0 && (uintptr_t)g_scaled % 16 == 0,
               "conv3x3_bwd_prepare: g, g_scaled and the workspace must be aligned to 16 bytes");
    hipStream_t st = (hipStream_t)stream;
    float *sums = (float *)workspace, *amax = (float *)((char *)workspace + p.amax);
    hipLaunchKernelGGL(k_prep_partial, dim3(p.nprep, p.ncb), dim3(NT), 0, st, g, p.npix, p.pchunk, Co, sums, amax);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_prep_finish, dim3(p.ncb), dim3(NT), 0, st, sums, amax, p.nprep, p.ncb, Co, grad_bias, scale2);
    PS_LAUNCH_CHECK();
    const size_t n4 = (size_t)p.npix * Co / 4;
    hipLaunchKernelGGL(k_scale, dim3(stream_grid(n4)), dim3(NT), 0, st, (const f32x4 *)g, n4, scale2, 0, (f32x4 *)g_scaled);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_conv3x3_grad_weight_f16x3(const float *x, const float *g_scaled, const float *scale2, int B, int H, int W, int Ci, int Co,
                                 float *grad_weight, int *overflow, void *workspace, size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(x && g_scaled && scale2 && grad_weight && overflow && workspace, "conv3x3_grad_weight: null pointer");
    PS_REQUIRE(sizes_ok(B, H, W, Ci, Co), "conv3x3_grad_weight: B = %d, H = %d, W = %d, Ci = %d, Co = %d: H and W multiples of 16, Ci and Co "
               "multiples of 64, H*W*max(Ci,Co) < 2^31 and B*H*W <= 2^30 required", B, H, W, Ci, Co);
    const Plan p = make_plan(B, H, W, Ci, Co);
    PS_REQUIRE(workspace_bytes >= p.bytes, "conv3x3_grad_weight: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    PS_REQUIRE((uintptr_t)workspace % 16 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)g_scaled % 16 == 0 && (uintptr_t)grad_weight % 16 == 0,
               "conv3x3_grad_weight: x, g_scaled, grad_weight and the workspace must be aligned to 16 bytes");
    PS_REQUIRE(p.blocks <= 65535, "conv3x3_grad_weight: Ci = %d, Co = %d exceed the launch grid", Ci, Co);
    hipStream_t st = (hipStream_t)stream;
    GwArgs a;
    a.x = x; a.g = g_scaled; a.part = (float *)workspace; a.overflow = overflow;
    a.H = H; a.W = W; a.Ci = Ci; a.Co = Co;
    a.tiles_x = W / TW; a.tiles_per_frame = (H / TR) * a.tiles_x; a.ntiles = p.ntiles; a.chunk = p.chunk; a.ncib = Ci / CB;
    hipLaunchKernelGGL(k_grad_weight_parts, dim3(p.parts, p.blocks), dim3(NT), 0, st, a);
    PS_LAUNCH_CHECK();
    const size_t n4 = (size_t)9 * Co * Ci / 4;
    hipLaunchKernelGGL(k_grad_weight_sum, dim3((unsigned)((n4 + NT - 1) / NT)), dim3(NT), 0, st, (const f32x4 *)workspace, p.parts, n4, scale2,
                       (f32x4 *)grad_weight);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_conv3x3_bwd_unscale_f32(float *y, size_t n, const float *scale2, void *stream)
{
    PS_REQUIRE(y && scale2, "conv3x3_bwd_unscale: null pointer");
    PS_REQUIRE(n % 4 == 0 && (uintptr_t)y % 16 == 0, "conv3x3_bwd_unscale: n = %zu a multiple of 4 and y aligned to 16 bytes required", n);
    if (n == 0) return PS_OK;
    hipLaunchKernelGGL(k_scale, dim3(stream_grid(n / 4)), dim3(NT), 0, (hipStream_t)stream, (const f32x4 *)y, n / 4, scale2, 1, (f32x4 *)y);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
