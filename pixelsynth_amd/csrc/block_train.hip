// block_train.hip -- what a decoder block needs in training mode between its 3 x 3 convolutions (conv_bwd.hip) and its norms
// (norm_train.hip), for gfx950 (MI355X): the weight / bias gradient of the 1 x 1 projection on the other branch and the adjoints of the
// two resampling passes that join the branches (nets.hip: k_upsample_add, k_pool_add).  Behind the C ABI of
// include/pixelsynth_block_train.h (libpixelsynth_block_train.so, beside libpixelsynth_hip.so whose set of exports it leaves as it is).
//
// k_grad_weight: dW (Co, Ci) = g^T (Co, P) . x (P, Ci), a GEMM whose K is the pixels, on v_mfma_f32_16x16x4_f32 (an fp32 fma chain).
// Both operands are channels-last, so K runs along the SLOW axis of both -- and an MFMA does not care which pixel is which k, nor which
// channel is which row, as long as A and B agree on the pixels.  Lane (i, kk) = (lane & 15, lane >> 4) reads the 16 bytes
// g[p0 + kk][64 q + 4 i ..] and x[p0 + kk][64 q' + 4 i ..] -- one row segment each, straight into registers, read once -- and element ja
// of the one with element jb of the other is an MFMA whose row m stands for output channel 64 q + 4 m + ja, column n for input channel
// 64 q' + 4 n + jb, k for pixel p0 + k: 16 MFMAs per pair of loads give the 64 x 64 block (q, q') its four pixels.  A workgroup pairs
// TO chunks of g with TC of x (TO TC <= 2: 128 accumulator registers); its eight wavefronts take the part's groups of four pixels in
// turn and are added through LDS in ascending order; the parts (a function of the sizes alone, see the header) go to the workspace and
// k_sum_parts adds them in ascending order.  The bias sums ride on the same registers of g (vector adds beside 32 MFMAs).
// k_upsample_add_bwd, k_pool_add_bwd: gathers, 16 bytes per lane, one fixed order of summation (the header spells it out).
// No atomics anywhere.
#include "ps_common.h"

#include "../../include/pixelsynth_block_train.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WAVES = PS_BLOCK_TRAIN_WAVES, THREADS = 64 * WAVES;

struct GwPlan {
    int TO, TC, tiles_o, tiles_c, parts;
    size_t part_pix, stride, bytes;      // pixels of a part; floats of a part's slab (Co Ci + Co); bytes of the workspace
};

inline bool gw_sizes_ok(size_t npix, int Ci, int Co)
{
    return npix > 0 && npix % 16 == 0 && Ci > 0 && Co > 0 && Ci % 16 == 0 && Co % 16 == 0 && Ci <= PS_BLOCK_TRAIN_MAX_CHANNELS &&
           Co <= PS_BLOCK_TRAIN_MAX_CHANNELS;
}

// The split of the pixels and of the output: a function of the sizes alone (the header's formula)
inline GwPlan gw_plan(size_t npix, int Ci, int Co)
{
    GwPlan p;
    const int nbo = (Co + 63) / 64, nbc = (Ci + 63) / 64;
    p.TO = nbo % 2 == 0 ? 2 : 1;
    p.TC = p.TO == 1 && nbc % 2 == 0 ? 2 : 1;
    p.tiles_o = nbo / p.TO;
    p.tiles_c = nbc / p.TC;
    const int tiles = p.tiles_o * p.tiles_c;
    const size_t target = std::min<size_t>(PS_BLOCK_TRAIN_MAX_PARTS, std::max(1, 512 / tiles));
    const size_t steps = npix / 16;
    p.part_pix = std::max<size_t>(PS_BLOCK_TRAIN_MIN_PART, 16 * ((steps + target - 1) / target));
    p.parts = (int)((npix + p.part_pix - 1) / p.part_pix);
    p.stride = (size_t)Co * Ci + Co;
    p.bytes = ps::align_up((size_t)p.parts * p.stride * sizeof(float), 256);
    return p;
}

struct GwArgs {
    const float *x, *g;
    size_t npix, part_pix, stride;
    int Ci, Co, tiles_c;
    float *out;          // part 0's (Co, Ci) block, part p's `stride` floats on
    float *bias_out;     // part 0's (Co) sums, or null
};

template <int TO, int TC>
__global__ __launch_bounds__(THREADS) void k_grad_weight(GwArgs a)
{
    __shared__ f32x4 sAcc[TO * TC * 16][64];
    __shared__ f32x4 sBias[WAVES][4][TO][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, kk = lane >> 4;
    const int Ci = a.Ci, Co = a.Co;
    const int oq0 = ((int)blockIdx.x / a.tiles_c) * TO, cq0 = ((int)blockIdx.x % a.tiles_c) * TC;      // the first 64-channel chunks
    const size_t part = blockIdx.y, p_lo = part * a.part_pix, p_hi = std::min(a.npix, p_lo + a.part_pix);
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};

    // this lane's four channels of every chunk; a chunk that ends early (a count that is no multiple of 64) reads channel 0 and uses zeros
    bool on_g[TO], on_x[TC];
    const float *gp[TO], *xp[TC];
#pragma unroll
    for (int t = 0; t < TO; ++t) {
        const int o = (oq0 + t) * 64 + 4 * i;
        on_g[t] = o < Co;
        gp[t] = a.g + (on_g[t] ? o : 0);
    }
#pragma unroll
    for (int t = 0; t < TC; ++t) {
        const int c = (cq0 + t) * 64 + 4 * i;
        on_x[t] = c < Ci;
        xp[t] = a.x + (on_x[t] ? c : 0);
    }

    f32x4 acc[TO][TC][4][4];
    f32x4 bs[TO];
#pragma unroll
    for (int to = 0; to < TO; ++to) {
        bs[to] = zero;
#pragma unroll
        for (int tc = 0; tc < TC; ++tc)
#pragma unroll
            for (int ja = 0; ja < 4; ++ja)
#pragma unroll
                for (int jb = 0; jb < 4; ++jb) acc[to][tc][ja][jb] = zero;
    }

    // (the bounds of a part are multiples of 16 pixels: a group of four is inside it or not, the same for every lane)
    // and the next group's rows are on their way while this one's 16 TO TC MFMAs run)
    f32x4 gv[TO], xv[TC], gn[TO], xn[TC];
    size_t q = p_lo + 4 * wave;
#pragma unroll
    for (int t = 0; t < TO; ++t) gn[t] = q < p_hi ? *(const f32x4 *)(gp[t] + (q + kk) * (size_t)Co) : zero;
#pragma unroll
    for (int t = 0; t < TC; ++t) xn[t] = q < p_hi ? *(const f32x4 *)(xp[t] + (q + kk) * (size_t)Ci) : zero;
    for (; q < p_hi; q += 4 * WAVES) {
#pragma unroll
        for (int t = 0; t < TO; ++t) gv[t] = on_g[t] ? gn[t] : zero;
#pragma unroll
        for (int t = 0; t < TC; ++t) xv[t] = on_x[t] ? xn[t] : zero;
        const size_t pn = q + 4 * WAVES + kk;
        if (q + 4 * WAVES < p_hi) {
#pragma unroll
            for (int t = 0; t < TO; ++t) gn[t] = *(const f32x4 *)(gp[t] + pn * (size_t)Co);
#pragma unroll
            for (int t = 0; t < TC; ++t) xn[t] = *(const f32x4 *)(xp[t] + pn * (size_t)Ci);
        }
#pragma unroll
        for (int to = 0; to < TO; ++to) {
            bs[to] = bs[to] + gv[to];
#pragma unroll
            for (int tc = 0; tc < TC; ++tc)
#pragma unroll
                for (int ja = 0; ja < 4; ++ja)
#pragma unroll
                    for (int jb = 0; jb < 4; ++jb)
                        acc[to][tc][ja][jb] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[to][ja], xv[tc][jb], acc[to][tc][ja][jb], 0, 0, 0);
        }
    }

    // the wavefronts in ascending order; slot [(tile, ja, r)][lane] holds the four input channels jb = 0 .. 3 of output row 16 kk + 4 r + ja
    const bool with_bias = a.bias_out != nullptr && cq0 == 0;
    if (with_bias) {
#pragma unroll
        for (int t = 0; t < TO; ++t) sBias[wave][kk][t][i] = bs[t];
    }
    for (int w = 0; w < WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int to = 0; to < TO; ++to)
#pragma unroll
                for (int tc = 0; tc < TC; ++tc)
#pragma unroll
                    for (int ja = 0; ja < 4; ++ja)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int idx = ((to * TC + tc) * 4 + ja) * 4 + r;
                            const f32x4 v = {acc[to][tc][ja][0][r], acc[to][tc][ja][1][r], acc[to][tc][ja][2][r], acc[to][tc][ja][3][r]};
                            sAcc[idx][lane] = w == 0 ? v : sAcc[idx][lane] + v;
                        }
        }
        __syncthreads();
    }

    float *dst = a.out + part * a.stride;
    for (int e = tid; e < TO * TC * 16 * 64; e += THREADS) {
        const int idx = e >> 6, l = e & 63, r = idx & 3, ja = (idx >> 2) & 3, tile = idx >> 4, to = tile / TC, tc = tile % TC;
        const int o = (oq0 + to) * 64 + 16 * (l >> 4) + 4 * r + ja, c = (cq0 + tc) * 64 + 4 * (l & 15);
        if (o < Co && c < Ci) *(f32x4 *)(dst + (size_t)o * Ci + c) = sAcc[idx][l];
    }
    if (with_bias && tid < TO * 16) {
        const int t = tid >> 4, ii = tid & 15, o = (oq0 + t) * 64 + 4 * ii;
        f32x4 v = zero;
        for (int w = 0; w < WAVES; ++w)
#pragma unroll
            for (int k = 0; k < 4; ++k) v = (w == 0 && k == 0) ? sBias[0][0][t][ii] : v + sBias[w][k][t][ii];
        if (o < Co) *(f32x4 *)(a.bias_out + part * a.stride + o) = v;
    }
}

// out[e] = slab[0][e] + slab[1][e] + ... in ascending part; e < nw4: the weight's gradient, from there on the bias's
__global__ __launch_bounds__(256) void k_sum_parts(const f32x4 *__restrict__ slab, int parts, size_t stride4, int n4, int nw4,
                                                   f32x4 *__restrict__ out_w, f32x4 *__restrict__ out_b)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n4) return;
    f32x4 v = slab[e];
#pragma unroll 8
    for (int p = 1; p < parts; ++p) v = v + slab[(size_t)p * stride4 + e];
    if (e < nw4)
        out_w[e] = v;
    else
        out_b[e - nw4] = v;
}

// One axis of the bilinear x2's adjoint: the (at most four) output indices 2 i - 1 .. 2 i + 2 that input index i of n hears from, their
// weights, and which of them exist (the header's table)
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

__global__ __launch_bounds__(256) void k_upsample_add_bwd(const f32x4 *__restrict__ g, int H, int W, int C4, size_t total4,
                                                          f32x4 *__restrict__ out)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total4; e += (size_t)gridDim.x * 256) {
        const int c4 = (int)(e % C4);
        size_t p = e / C4;
        const int x = (int)(p % W);
        p /= W;
        const int y = (int)(p % H);
        const size_t f = p / H;
        const UpAxis ay = up_axis(y, H), ax = up_axis(x, W);
        const f32x4 *gf = g + f * 4 * H * W * C4 + c4;
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
        out[e] = acc;
    }
}

__global__ __launch_bounds__(256) void k_pool_add_bwd(const f32x4 *__restrict__ g, int H, int W, int C4, size_t total4,
                                                      f32x4 *__restrict__ out)
{
    const int Ho = H / 2, Wo = W / 2;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total4; e += (size_t)gridDim.x * 256) {
        const int c4 = (int)(e % C4);
        size_t p = e / C4;
        const int xx = (int)(p % W);
        p /= W;
        const int yy = (int)(p % H);
        const size_t f = p / H;
        // outputs yy / 2 and, for an odd yy, (yy + 1) / 2 where that is one
        const int ny = (yy & 1) && (yy + 1) / 2 < Ho ? 2 : 1, nx = (xx & 1) && (xx + 1) / 2 < Wo ? 2 : 1;
        const f32x4 *gf = g + (f * Ho * Wo + (size_t)(yy / 2) * Wo + xx / 2) * C4 + c4;
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int r = 0; r < ny; ++r)
            for (int c = 0; c < nx; ++c) acc = acc + gf[((size_t)r * Wo + c) * C4];
        const float ninth = 1.0f / 9.0f;
        out[e] = acc * ninth;
    }
}

unsigned grid_for(size_t total4) { return (unsigned)std::min<size_t>((total4 + 255) / 256, 256 * 32); }

using ps::aligned16;

template <int TO, int TC> int launch_grad_weight(const GwArgs &a, const GwPlan &p, hipStream_t st)
{
    hipLaunchKernelGGL((k_grad_weight<TO, TC>), dim3(p.tiles_o * p.tiles_c, p.parts), dim3(THREADS), 0, st, a);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // namespace

extern "C" {

const char *ps_block_train_last_error(void) { return ps::last_error_ref().c_str(); }

int ps_conv1x1_grad_weight_parts(size_t npix, int Ci, int Co) { return gw_sizes_ok(npix, Ci, Co) ? gw_plan(npix, Ci, Co).parts : 0; }

size_t ps_conv1x1_grad_weight_workspace_bytes(size_t npix, int Ci, int Co)
{
    return gw_sizes_ok(npix, Ci, Co) ? gw_plan(npix, Ci, Co).bytes : 0;
}

int ps_conv1x1_grad_weight_f32(const float *x, const float *g, size_t npix, int Ci, int Co, float *grad_weight, float *grad_bias,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    PS_REQUIRE(x && g && grad_weight, "conv1x1_grad_weight: null pointer");
    PS_REQUIRE(gw_sizes_ok(npix, Ci, Co),
               "conv1x1_grad_weight: Ci and Co multiples of 16 up to %d and npix a positive multiple of 16 required (npix = %zu, Ci = %d, Co = %d)",
               PS_BLOCK_TRAIN_MAX_CHANNELS, npix, Ci, Co);
    PS_REQUIRE(aligned16(x) && aligned16(g) && aligned16(grad_weight) && aligned16(grad_bias),
               "conv1x1_grad_weight: buffers must be aligned to 16 bytes");
    const GwPlan p = gw_plan(npix, Ci, Co);
    PS_REQUIRE(workspace, "conv1x1_grad_weight: null pointer (workspace)");
    PS_REQUIRE(workspace_bytes >= p.bytes, "conv1x1_grad_weight: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    PS_REQUIRE(aligned16(workspace), "conv1x1_grad_weight: the workspace must be aligned to 16 bytes");
    hipStream_t st = (hipStream_t)stream;
    float *slab = (float *)workspace;
    const size_t nw = (size_t)Co * Ci;
    GwArgs a{x, g, npix, p.part_pix, p.stride, Ci, Co, p.tiles_c, slab, grad_bias ? slab + nw : nullptr};
    if (p.parts == 1) {      // nothing to add: the one part is the result
        a.out = grad_weight;
        a.bias_out = grad_bias;
    }
    int rc;
    if (p.TO == 2)
        rc = launch_grad_weight<2, 1>(a, p, st);
    else if (p.TC == 2)
        rc = launch_grad_weight<1, 2>(a, p, st);
    else
        rc = launch_grad_weight<1, 1>(a, p, st);
    if (rc != PS_OK || p.parts == 1) return rc;
    const int nw4 = (int)(nw / 4), n4 = nw4 + (grad_bias ? Co / 4 : 0);
    hipLaunchKernelGGL(k_sum_parts, dim3((n4 + 255) / 256), dim3(256), 0, st, (const f32x4 *)slab, p.parts, p.stride / 4, n4, nw4,
                       (f32x4 *)grad_weight, (f32x4 *)grad_bias);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_upsample_add_bwd_nhwc_f32(const float *g, int B, int H, int W, int C, float *grad_in, void *stream)
{
    PS_REQUIRE(g && grad_in, "upsample_add_bwd: null pointer");
    PS_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "upsample_add_bwd: B, H, W >= 1 and C a positive multiple of 4 required (B = %d, H = %d, W = %d, C = %d)",
               B, H, W, C);
    PS_REQUIRE(H < (1 << 30) && W < (1 << 30), "upsample_add_bwd: frame too large");
    PS_REQUIRE(aligned16(g) && aligned16(grad_in), "upsample_add_bwd: buffers must be aligned to 16 bytes");
    const size_t total4 = (size_t)B * H * W * (C / 4);
    hipLaunchKernelGGL(k_upsample_add_bwd, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, (const f32x4 *)g, H, W, C / 4, total4,
                       (f32x4 *)grad_in);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_pool_add_bwd_nhwc_f32(const float *g, int B, int H, int W, int C, float *grad_in, void *stream)
{
    PS_REQUIRE(g && grad_in, "pool_add_bwd: null pointer");
    PS_REQUIRE(B > 0 && H > 1 && W > 1 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 4 == 0,
               "pool_add_bwd: even H, W and C a positive multiple of 4 required (B = %d, H = %d, W = %d, C = %d)", B, H, W, C);
    PS_REQUIRE(aligned16(g) && aligned16(grad_in), "pool_add_bwd: buffers must be aligned to 16 bytes");
    const size_t total4 = (size_t)B * H * W * (C / 4);
    hipLaunchKernelGGL(k_pool_add_bwd, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, (const f32x4 *)g, H, W, C / 4, total4,
                       (f32x4 *)grad_in);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
