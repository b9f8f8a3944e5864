// lmconv_bwd.hip -- the backward pass of the locally masked convolution for gfx950 (MI355X): the gradients with respect to weight and
// bias, and the adjoint mask with which the gradient with respect to the input is a locally masked convolution itself.
//
// Behind the C ABI of include/pixelsynth_lmconv_bwd.h (libpixelsynth_lmconv_bwd.so, beside libpixelsynth_hip.so whose set of exports
// it leaves as it is).
//
//   grad_W[o,c,t] = sum_n g[n,o] * (m[t,n] * xpad[n + off(t), c]),  n = (b,l) over the N = B*L locations
//
// is, per tap t, a GEMM (Co x N) (N x Ci) whose reduction runs over the locations:
//   k_to_cl               g and x as channels-last copies (N, C padded to 16 with zeros), through a 32 x 32 LDS tile: per location
//                         16 consecutive floats are then one operand row of v_mfma_f32_16x16x4_f32 (lane l holds A[l&15][l>>4] and
//                         B[l>>4][l&15]).
//   k_grad_weight_parts   one wave per (part, tap, 32 output channels, 32 input channels): a 2 x 2 block of 16 x 16 accumulator tiles
//                         -- four independent chains, so the MFMA's 40-cycle dependent latency never waits on its 32-cycle issue, and
//                         two A and two B operand loads feed four MFMAs.  The B operand is the row of x at the tap's shifted location
//                         scaled by the mask value of (t, l); outside the grid, past the last location and past the last channel tile
//                         it is an exact 0 (the lane loads location 0 or the block's first tile instead, never outside a buffer).
//                         Four steps' operands are loaded, branch-free, before their sixteen MFMAs.  The N locations are split into `parts` consecutive ranges so
//                         that the 9 * ceil(Co/32) * ceil(Ci/32) wave tasks fill the device; each part writes its tiles to the workspace.
//   k_grad_weight_sum     adds the partial tiles in ascending order of the part and writes (Co,Ci,3,3).
//   k_grad_bias           one workgroup per output channel over g as it lies (NCHW).
//   k_adjoint_mask        m'[b,t,p] = m[b,8-t,p+off(t)] inside the grid, 0 outside.
// No atomics anywhere: every sum has one fixed order.
#include "ps_common.h"

#include "../../include/pixelsynth_lmconv_bwd.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int TILE = 16, BLOCK = 2 * TILE;      // channels of an MFMA tile / of a wave's 2 x 2 block of them
constexpr int KSTEP = 4;                        // locations per MFMA
constexpr int TARGET_WAVES = 256 * 4 * 4;       // four waves on every SIMD of 256 compute units
constexpr int DEPTH = 4;                        // steps whose operand loads a wave issues before their MFMAs
constexpr int MAX_LOCATIONS = 1 << 30;

struct Plan {
    int N, Cop, Cip, obk, cbk, ksteps, parts, chunk;
    size_t gcl, xcl, part, bytes;               // byte offsets into the workspace, and its size
};

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// The split of the reduction and the layout of the workspace: a function of the sizes alone
inline Plan make_plan(int B, int Ci, int Co, int H, int W)
{
    Plan p;
    p.N = B * H * W;
    p.Cop = ceil_div(Co, TILE) * TILE;
    p.Cip = ceil_div(Ci, TILE) * TILE;
    p.obk = ceil_div(p.Cop, BLOCK);
    p.cbk = ceil_div(p.Cip, BLOCK);
    p.ksteps = ceil_div(p.N, KSTEP);
    const long long tasks = 9LL * p.obk * p.cbk;
    long long want = (TARGET_WAVES + tasks - 1) / tasks;
    if (want > PS_LMCONV_BWD_MAX_PARTS) want = PS_LMCONV_BWD_MAX_PARTS;
    if (want > p.ksteps) want = p.ksteps;
    if (want < 1) want = 1;
    p.chunk = ceil_div(p.ksteps, (int)want);
    p.parts = ceil_div(p.ksteps, p.chunk);      // (no empty part)
    p.gcl = 0;
    p.xcl = ps::align_up(p.gcl + (size_t)p.N * p.Cop * sizeof(float), 256);
    p.part = ps::align_up(p.xcl + (size_t)p.N * p.Cip * sizeof(float), 256);
    p.bytes = ps::align_up(p.part + (size_t)p.parts * 9 * p.Cop * p.Cip * sizeof(float), 256);
    return p;
}

inline bool sizes_ok(int B, int Ci, int Co, int H, int W)
{
    return B >= 1 && Ci >= 1 && Co >= 1 && H >= 1 && W >= 1 && (long long)B * H * W <= MAX_LOCATIONS && Ci <= (1 << 20) && Co <= (1 << 20);
}

// in (B,C,L) -> out (B*L,Cp), Cp a multiple of 16 >= C, channels C .. Cp-1 zero.  grid (ceil(L/32), ceil(Cp/32), B), block (32,8)
__global__ __launch_bounds__(256) void k_to_cl(const float *__restrict__ in, int C, int Cp, int L, float *__restrict__ out)
{
    __shared__ float tile[32][33];
    const int tx = threadIdx.x, ty = threadIdx.y, b = blockIdx.z;
    const int l0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int c = c0 + ty + k, l = l0 + tx;
        tile[ty + k][tx] = (c < C && l < L) ? in[((size_t)b * C + c) * L + l] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int l = l0 + ty + k, c = c0 + tx;
        if (l < L && c < Cp) out[((size_t)b * L + l) * Cp + c] = tile[tx][ty + k];
    }
}

// One wave per (part, tap, block of 32 output channels, block of 32 input channels), the input-channel block fastest: the four waves
// of a workgroup mostly share their rows of g.  No LDS, no barrier: a wave without a task leaves.
__global__ __launch_bounds__(THREADS) void k_grad_weight_parts(const float *__restrict__ gcl, const float *__restrict__ xcl,
                                                               const float *__restrict__ mask, size_t mstride, int B, int H, int W,
                                                               int dil, int Cop, int Cip, int obk, int cbk, int parts, int chunk,
                                                               int ksteps, float *__restrict__ part_out)
{
    const int lane = threadIdx.x & 63;
    long long w = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (w >= 9LL * parts * obk * cbk) return;
    const int cb = (int)(w % cbk);
    w /= cbk;
    const int ob = (int)(w % obk);
    w /= obk;
    const int t = (int)(w % 9), p = (int)(w / 9);
    const int L = H * W, N = B * L;
    const int kr = lane >> 4, col = lane & 15;
    const int di = (t / 3 - 1) * dil, dj = (t % 3 - 1) * dil;
    const int o0 = ob * BLOCK + col, c0 = cb * BLOCK + col;
    const bool o_hi = ob * BLOCK + TILE < Cop, c_hi = cb * BLOCK + TILE < Cip;     // (the second tile of a block may lie past the channels)
    const int s0 = p * chunk, s1 = min(s0 + chunk, ksteps);
    int n = s0 * KSTEP + kr;                    // this lane's location: row k = lane >> 4 of each step's four
    int b = n / L, i = (n - b * L) / W, j = n - b * L - i * W;
    f32x4 acc00 = {0, 0, 0, 0}, acc01 = acc00, acc10 = acc00, acc11 = acc00;
    const float *mt = mask + (size_t)t * L;
    const int o1 = o_hi ? o0 + TILE : o0, c1 = c_hi ? c0 + TILE : c0;              // (a tile past the channels reads the first one's, unused)
    for (int s = s0; s < s1; s += DEPTH) {
        // The operands of DEPTH steps first, without a branch, so that their loads are in flight together: a step past the part's
        // end, a location past the last and a tap outside the grid load location 0 instead and are zeroed below (fma(0, 0, acc) = acc)
        float a0[DEPTH], a1[DEPTH], x0[DEPTH], x1[DEPTH], mv[DEPTH];
        bool open[DEPTH];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            const bool valid = s + u < s1 && n < N;
            const int ii = i + di, jj = j + dj;
            open[u] = valid && (unsigned)ii < (unsigned)H && (unsigned)jj < (unsigned)W;
            const float *gr = gcl + (size_t)(valid ? n : 0) * Cop;
            const float *xr = xcl + (open[u] ? (size_t)b * L + ii * W + jj : (size_t)0) * Cip;
            a0[u] = gr[o0];
            a1[u] = gr[o1];
            mv[u] = mt[open[u] ? (size_t)b * mstride + i * W + j : (size_t)0];
            x0[u] = xr[c0];
            x1[u] = xr[c1];
            if (!valid) a0[u] = a1[u] = 0.0f;
            n += KSTEP;
            j += KSTEP;
            while (j >= W) { j -= W; ++i; }
            while (i >= H) { i -= H; ++b; }
        }
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {           // (ascending locations: each accumulator stays one chain)
            const float b0 = open[u] ? mv[u] * x0[u] : 0.0f, b1 = open[u] && c_hi ? mv[u] * x1[u] : 0.0f;
            const float a1u = o_hi ? a1[u] : 0.0f;
            acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[u], b0, acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[u], b1, acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1u, b0, acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1u, b1, acc11, 0, 0, 0);
        }
    }
    // C/D: lane holds rows 4 (lane >> 4) + r, column lane & 15
    float *out = part_out + ((size_t)p * 9 + t) * Cop * (size_t)Cip;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = ob * BLOCK + 4 * kr + r;
        out[(size_t)o * Cip + c0] = acc00[r];
        if (c_hi) out[(size_t)o * Cip + c0 + TILE] = acc01[r];
        if (o_hi) {
            out[(size_t)(o + TILE) * Cip + c0] = acc10[r];
            if (c_hi) out[(size_t)(o + TILE) * Cip + c0 + TILE] = acc11[r];
        }
    }
}

// grad_W[o,c,t] = part 0 + part 1 + ... in that order; thread e = (t, o, c), c fastest (the reads of a wave are consecutive)
__global__ __launch_bounds__(THREADS) void k_grad_weight_sum(const float *__restrict__ part, int parts, int Co, int Ci, int Cop, int Cip,
                                                             float *__restrict__ gw)
{
    const long long e = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= 9LL * Co * Ci) return;
    const int c = (int)(e % Ci), o = (int)((e / Ci) % Co), t = (int)(e / ((long long)Ci * Co));
    const size_t stride = (size_t)9 * Cop * Cip;
    const float *src = part + ((size_t)t * Cop + o) * Cip + c;
    float s = src[0];
    for (int p = 1; p < parts; ++p) s += src[(size_t)p * stride];
    gw[((size_t)o * Ci + c) * 9 + t] = s;
}

__global__ __launch_bounds__(THREADS) void k_grad_bias(const float *__restrict__ g, int B, int Co, int L, float *__restrict__ gb)
{
    __shared__ float sh[THREADS];
    const int o = blockIdx.x, t = threadIdx.x;
    float s = 0.0f;
    for (int b = 0; b < B; ++b) {
        const float *row = g + ((size_t)b * Co + o) * L;
        for (int l = t; l < L; l += THREADS) s += row[l];
    }
    sh[t] = s;
    __syncthreads();
    for (int off = THREADS / 2; off > 0; off >>= 1) {
        if (t < off) sh[t] += sh[t + off];
        __syncthreads();
    }
    if (t == 0) gb[o] = sh[0];
}

__global__ __launch_bounds__(THREADS) void k_adjoint_mask(const float *__restrict__ m, int H, int W, int dil, long long total,
                                                          float *__restrict__ out)
{
    const long long e = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= total) return;
    const int L = H * W;
    const int p = (int)(e % L), t = (int)((e / L) % 9);
    const long long b = e / (9LL * L);
    const int i = p / W + (t / 3 - 1) * dil, j = p % W + (t % 3 - 1) * dil;
    float v = 0.0f;
    if ((unsigned)i < (unsigned)H && (unsigned)j < (unsigned)W) v = m[(b * 9 + (8 - t)) * L + i * W + j];
    out[e] = v;
}

}  // namespace

extern "C" {

const char *ps_lmconv_bwd_last_error(void) { return ps::last_error_ref().c_str(); }

size_t ps_lmconv_bwd_workspace_bytes(int B, int Ci, int Co, int H, int W)
{
    if (!sizes_ok(B, Ci, Co, H, W)) return 0;
    return make_plan(B, Ci, Co, H, W).bytes;
}

int ps_lmconv_grad_weight_f32(const float *x, const float *grad_y, const float *mask, size_t mask_batch_stride, int B, int Ci, int Co,
                              int H, int W, int dilation, float *grad_weight, float *grad_bias, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(grad_y, "lmconv_grad_weight: null pointer (grad_y)");
    PS_REQUIRE(grad_weight || grad_bias, "lmconv_grad_weight: no output (grad_weight and grad_bias are both NULL)");
    PS_REQUIRE(!grad_weight || (x && mask && workspace), "lmconv_grad_weight: null pointer (grad_weight needs x, mask and the workspace)");
    PS_REQUIRE(B >= 1 && Ci >= 1 && Co >= 1 && H >= 1 && W >= 1, "lmconv_grad_weight: B = %d, Ci = %d, Co = %d, H = %d, W = %d, expected all >= 1",
               B, Ci, Co, H, W);
    PS_REQUIRE(sizes_ok(B, Ci, Co, H, W), "lmconv_grad_weight: B*H*W = %lld locations, Ci = %d, Co = %d: more than %d locations or 2^20 channels",
               (long long)B * H * W, Ci, Co, MAX_LOCATIONS);
    PS_REQUIRE(dilation >= 1 && dilation <= (1 << 20), "lmconv_grad_weight: dilation = %d, expected >= 1", dilation);
    const int L = H * W;
    PS_REQUIRE(mask_batch_stride == 0 || mask_batch_stride == (size_t)9 * L, "lmconv_grad_weight: mask_batch_stride = %zu, expected 0 or 9*H*W = %zu",
               mask_batch_stride, (size_t)9 * L);
    const Plan p = make_plan(B, Ci, Co, H, W);
    PS_REQUIRE(!grad_weight || workspace_bytes >= p.bytes, "lmconv_grad_weight: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    PS_REQUIRE(!grad_weight || (uintptr_t)workspace % 16 == 0, "lmconv_grad_weight: the workspace must be aligned to 16 bytes");
    const long long waves = 9LL * p.parts * p.obk * p.cbk;
    PS_REQUIRE(!grad_weight || (B <= 65535 && waves / WAVES < (1LL << 31) - 1), "lmconv_grad_weight: B = %d, Ci = %d, Co = %d exceed the launch grid",
               B, Ci, Co);
    hipStream_t st = (hipStream_t)stream;
    if (grad_bias) {
        hipLaunchKernelGGL(k_grad_bias, dim3(Co), dim3(THREADS), 0, st, grad_y, B, Co, L, grad_bias);
        PS_LAUNCH_CHECK();
    }
    if (!grad_weight) return PS_OK;
    float *gcl = (float *)((char *)workspace + p.gcl), *xcl = (float *)((char *)workspace + p.xcl);
    float *part = (float *)((char *)workspace + p.part);
    hipLaunchKernelGGL(k_to_cl, dim3(ceil_div(L, 32), ceil_div(p.Cop, 32), B), dim3(32, 8), 0, st, grad_y, Co, p.Cop, L, gcl);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_to_cl, dim3(ceil_div(L, 32), ceil_div(p.Cip, 32), B), dim3(32, 8), 0, st, x, Ci, p.Cip, L, xcl);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_grad_weight_parts, dim3((unsigned)((waves + WAVES - 1) / WAVES)), dim3(THREADS), 0, st, gcl, xcl, mask,
                       mask_batch_stride, B, H, W, dilation, p.Cop, p.Cip, p.obk, p.cbk, p.parts, p.chunk, p.ksteps, part);
    PS_LAUNCH_CHECK();
    const long long elems = 9LL * Co * Ci;
    hipLaunchKernelGGL(k_grad_weight_sum, dim3((unsigned)((elems + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, part, p.parts, Co, Ci,
                       p.Cop, p.Cip, grad_weight);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_lmconv_adjoint_mask_f32(const float *mask, int Bm, int H, int W, int dilation, float *adjoint, void *stream)
{
    PS_REQUIRE(mask && adjoint, "lmconv_adjoint_mask: null pointer");
    PS_REQUIRE(mask != adjoint, "lmconv_adjoint_mask: the adjoint cannot be written in place");
    PS_REQUIRE(Bm >= 1 && H >= 1 && W >= 1, "lmconv_adjoint_mask: Bm = %d, H = %d, W = %d, expected all >= 1", Bm, H, W);
    PS_REQUIRE((long long)Bm * H * W <= MAX_LOCATIONS, "lmconv_adjoint_mask: Bm*H*W = %lld locations, more than %d", (long long)Bm * H * W,
               MAX_LOCATIONS);
    PS_REQUIRE(dilation >= 1 && dilation <= (1 << 20), "lmconv_adjoint_mask: dilation = %d, expected >= 1", dilation);
    const long long total = 9LL * Bm * H * W;
    hipLaunchKernelGGL(k_adjoint_mask, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, mask, H, W,
                       dilation, total, adjoint);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
