// ar_order.hip -- the generation orders of an AR plan on the device, for gfx950 (MI355X): what ps_ar_plan (csrc/host_order.cpp) works out on
// host threads from a copy of the background masks, from the masks where they already are.
//
// Behind the C ABI of include/pixelsynth_plan.h (libpixelsynth_plan.so, a library of its own beside libpixelsynth_hip.so).  Replaces, per
// frame and bit for bit, ps_generation_order + the order_loc / first-rank loop of ps_ar_plan:
//   pooling     host_order.cpp:122-130   a block is background iff all of its bytes are set, foreground iff none is
//   chamfer     host_order.cpp:26-55     cv2.distanceTransform(DIST_L2, 5) in 16.16 fixed point, on the foreground and on the background blocks
//   distance    host_order.cpp:135       D = (int64)((double)fd - (double)bd)
//   walk        host_order.cpp:58-82     the greedy frontier walk of custom_idx
//
// One workgroup of 256 threads per frame, one launch, nothing written but the four outputs:
//   1. all four waves pool the mask (16-byte loads, per-block sums by LDS atomics; the sums' total is bg_counts) and lay out the two
//      chamfer maps with their border of two cells;
//   2. wave 0 runs both distance transforms at once -- lanes 0..31 are the columns of the foreground map, lanes 32..63 those of the
//      background map.  Rows go one after the other; inside a row the only dependence is v[x] = min(c[x], v[x -+ 1] + m0), a min-plus
//      prefix scan over the 32 lanes of a map, exact in integers.  The backward pass's `best > metric[0]` test of the host only skips
//      work (best <= m0 is never above a neighbour + a metric >= m0), so it is dropped;
//   3. wave 0 walks the frontier.  A cell's key is (8192 - D) << 11 | r << 6 | c << 1 | region: keys are unique in (r, c), so the heap's
//      pop order (-D, r, c) is the order of the keys, and the start (first row-major argmax of D) is the smallest key of all.  D lies in
//      [-8192, 8192] (fd, bd are in [0, 8192.0]), the key in 26 bits.  Lane (r & 1) << 5 | c holds cell (r, c) in register slot r >> 1:
//      UNSEEN | key until a neighbour is taken, the key while it is in the frontier, TAKEN = 0x7FFFFFFF afterwards, 0xFFFFFFFF for a
//      cell outside a G < 32 grid -- so the frontier's smallest key is the smallest value of all while the frontier has a cell.  A step is
//      that minimum per lane, one DPP reduction over the wave, and the update of at most two slots.  Pushing a neighbour clears
//      its UNSEEN bit: a frontier or taken cell stays as it is, a cell outside the grid becomes a taken one.
#include "ps_common.h"

#include "../../include/pixelsynth_plan.h"

namespace {

constexpr int PLAN_THREADS = 256;
constexpr int PLAN_GMAX = 32;                       // the walk holds 32 x 32 cells in 16 registers per lane
constexpr int PLAN_SMAX = 4096;
constexpr uint32_t CH_INIT = 0x7FFFFFFF >> 2;       // Chamfer5::INIT
constexpr uint32_t CH_M0 = 65536u, CH_M1 = 91750u, CH_M2 = 143976u;   // 65536, lrint(1.4f * 65536), lrint(2.1969f * 65536) (checked below)
constexpr uint32_t NONE = 0xFFFFFFFFu, UNSEEN = 0x80000000u, TAKEN = 0x7FFFFFFFu;   // states of a cell of the walk (see above)
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));   // a lane's 16 cells: registers, also under an index that is a scalar
constexpr int MAP_STEP_MAX = PLAN_GMAX + 4, MAP_CELLS_MAX = MAP_STEP_MAX * MAP_STEP_MAX;

// minimum over the wave's 64 lanes (all active), in every lane's return value: four row_shr steps leave a row's minimum in its lane 15,
// row_bcast:15 / row_bcast:31 carry it on to lane 63.  Lanes a step does not write keep `old` = NONE.
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
#define PS_DPP_MIN(ctrl, rows) v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)NONE, (int)v, ctrl, rows, 0xf, false))
    PS_DPP_MIN(0x111, 0xf);   // row_shr:1
    PS_DPP_MIN(0x112, 0xf);   // row_shr:2
    PS_DPP_MIN(0x114, 0xf);   // row_shr:4
    PS_DPP_MIN(0x118, 0xf);   // row_shr:8
    PS_DPP_MIN(0x142, 0xa);   // row_bcast:15 into rows 1 and 3
    PS_DPP_MIN(0x143, 0xc);   // row_bcast:31 into rows 2 and 3
#undef PS_DPP_MIN
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// what one lane wrote to LDS is read by another lane of the same wave: the wave's LDS operations complete in order, this keeps the
// compiler from moving them across
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w)
{
    return (uint32_t)__popc((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u);
}

__global__ __launch_bounds__(PLAN_THREADS) void k_plan_order(const uint8_t *__restrict__ bg, int S, int G, int vec,
                                                             int32_t *__restrict__ order_loc, uint8_t *__restrict__ region,
                                                             int32_t *__restrict__ first_steps, int32_t *__restrict__ bg_counts)
{
    // the two chamfer maps; the per-block sums of the pooling pass lie in the first one until the maps are laid out
    __shared__ uint32_t s_map[2 * MAP_CELLS_MAX];
    __shared__ uint32_t s_rowbits[PLAN_GMAX];      // bit c of word r: block (r, c) is background
    __shared__ uint32_t s_total;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int L = G * G, blk = S / G, N = S * S;
    const int step = G + 4, cells = step * step;
    const uint8_t *f = bg + (size_t)b * N;
    uint32_t *cnt = s_map;

    for (int q = tid; q < L; q += PLAN_THREADS) cnt[q] = 0;
    if (tid < PLAN_GMAX) s_rowbits[tid] = 0;
    if (tid == 0) s_total = 0;
    __syncthreads();

    // ---- pooling: set bytes per block
    if (vec) {   // S % 16 == 0 and the masks are 16-byte aligned: a 16-byte piece lies in one row
        const bool by_word = (blk & 3) == 0;       // then a block's edge never cuts a 4-byte word
        for (int i = tid; i < N / 16; i += PLAN_THREADS) {
            const uint4 w4 = reinterpret_cast<const uint4 *>(f)[i];
            const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
            const int o = i * 16, y = o / S, x0 = o - y * S, by = y / blk;
            int bx = x0 / blk, rx = x0 - bx * blk;
            uint32_t acc = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (by_word) {
                    acc += nonzero_bytes(w[j]);
                    rx += 4;
                    if (rx == blk) {
                        if (acc) atomicAdd(&cnt[by * G + bx], acc);
                        acc = 0, rx = 0, ++bx;
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        acc += ((w[j] >> (8 * t)) & 0xffu) != 0;
                        if (++rx == blk) {
                            if (acc) atomicAdd(&cnt[by * G + bx], acc);
                            acc = 0, rx = 0, ++bx;
                        }
                    }
                }
            }
            if (acc) atomicAdd(&cnt[by * G + bx], acc);   // (a block wider than the piece)
        }
    } else {
        for (int p = tid; p < N; p += PLAN_THREADS)
            if (f[p]) {
                const int y = p / S, x = p - y * S;
                atomicAdd(&cnt[(y / blk) * G + x / blk], 1u);
            }
    }
    __syncthreads();

    // ---- block classes (each thread keeps those of its cells), region, bg_counts
    uint32_t is_fg = 0, is_bg = 0, ones = 0;       // bit j: cell tid + 256 j
#pragma unroll
    for (int j = 0; j < PLAN_GMAX * PLAN_GMAX / PLAN_THREADS; ++j) {
        const int q = tid + j * PLAN_THREADS;
        if (q < L) {
            const uint32_t n = cnt[q];
            const bool bgb = n == (uint32_t)(blk * blk);
            ones += n;
            is_fg |= (uint32_t)(n == 0) << j;
            is_bg |= (uint32_t)bgb << j;
            region[(size_t)b * L + q] = bgb;
            if (bgb) atomicOr(&s_rowbits[q / G], 1u << (q % G));
        }
    }
    if (ones) atomicAdd(&s_total, ones);
    __syncthreads();                               // (the sums are read: the maps may overwrite them)
    for (int i = tid; i < 2 * cells; i += PLAN_THREADS) s_map[i] = CH_INIT;
    __syncthreads();
    // Chamfer5::run(src): a cell starts at 0 where src is 0.  Map 0 has src = the foreground blocks, map 1 the background blocks;
    // every other inner cell is overwritten by the forward pass before it is read, INIT stands for "src set" until then.
#pragma unroll
    for (int j = 0; j < PLAN_GMAX * PLAN_GMAX / PLAN_THREADS; ++j) {
        const int q = tid + j * PLAN_THREADS;
        if (q < L) {
            const int at = (q / G + 2) * step + q % G + 2;
            if (!((is_fg >> j) & 1)) s_map[at] = 0;
            if (!((is_bg >> j) & 1)) s_map[cells + at] = 0;
        }
    }
    __syncthreads();
    if (tid == 0 && bg_counts) bg_counts[b] = (int32_t)s_total;
    if (tid >= 64) return;                         // (no barrier of the workgroup below)

    // ---- the two distance transforms, wave 0: lane = map << 5 | column
    const int lane = tid, x = lane & 31;
    uint32_t *M = s_map + (lane >> 5) * cells + 2;   // M[(y + 2) * step + x] = at(y, x)
    const bool in = x < G;
    for (int y = 0; y < G; ++y) {                  // forward
        uint32_t v = CH_INIT;
        if (in) {
            const uint32_t *r1 = M + (y + 1) * step + x, *r2 = M + y * step + x;    // rows y - 1, y - 2
            uint32_t c = min(min(r2[-1], r2[1]), min(r1[-2], r1[2])) + CH_M2;
            c = min(c, min(r1[-1], r1[1]) + CH_M1);
            c = min(c, r1[0] + CH_M0);
            if (M[(y + 2) * step + x] == 0) c = 0;
            v = min(c, CH_INIT + (uint32_t)(x + 1) * CH_M0);    // the border cell at(y, -1) = INIT, x + 1 cells away
        }
#pragma unroll
        for (int d = 1; d < 32; d <<= 1) {
            const uint32_t t = __shfl_up(v, d, 32);
            if (x >= d) v = min(v, t + (uint32_t)d * CH_M0);
        }
        if (in) M[(y + 2) * step + x] = v;
        wave_lds_sync();
    }
    for (int y = G - 1; y >= 0; --y) {             // backward
        uint32_t v = CH_INIT;
        if (in) {
            const uint32_t *r1 = M + (y + 3) * step + x, *r2 = M + (y + 4) * step + x;   // rows y + 1, y + 2
            uint32_t c = min(min(r2[-1], r2[1]), min(r1[-2], r1[2])) + CH_M2;
            c = min(c, min(r1[-1], r1[1]) + CH_M1);
            c = min(c, r1[0] + CH_M0);
            c = min(c, M[(y + 2) * step + x]);
            v = min(c, CH_INIT + (uint32_t)(G - x) * CH_M0);    // the border cell at(y, G) = INIT
        }
#pragma unroll
        for (int d = 1; d < 32; d <<= 1) {
            const uint32_t t = __shfl_down(v, d, 32);
            if (x + d < 32) v = min(v, t + (uint32_t)d * CH_M0);
        }
        if (in) M[(y + 2) * step + x] = v;
        wave_lds_sync();
    }

    // ---- keys: lane (r & 1) << 5 | c, slot r >> 1
    u32x16 v;
    const int c0 = lane & 31, rlow = lane >> 5;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int r = 2 * s + rlow;
        v[s] = NONE;
        if (r < G && c0 < G) {
            const int at = (r + 2) * step + c0 + 2;
            const float fd = (float)min(s_map[at], CH_INIT) * (1.0f / 65536.0f);
            const float bd = (float)min(s_map[cells + at], CH_INIT) * (1.0f / 65536.0f);
            const long long D = (long long)((double)fd - (double)bd);
            v[s] = UNSEEN | ((uint32_t)(8192 - D) << 11) | ((uint32_t)r << 6) | ((uint32_t)c0 << 1) | ((s_rowbits[r] >> c0) & 1u);
        }
    }

    // ---- the walk
    int32_t *out = order_loc + (size_t)b * L;
    int first = L, mine = 0;
    for (int i = 0; i < L; ++i) {
        uint32_t m = min(min(v[0], v[1]), min(v[2], v[3]));
        m = min(m, min(min(v[4], v[5]), min(v[6], v[7])));
        m = min(m, min(min(v[8], v[9]), min(v[10], v[11])));
        m = min(m, min(min(v[12], v[13]), min(v[14], v[15])));
        m = wave_min_u32(m) & TAKEN;               // (at the start every cell is UNSEEN: the smallest key of all)
        const int r = (m >> 6) & 31, c = (m >> 1) & 31;
        if ((m & 1u) && first == L) first = i;
        if (lane == (i & 63)) mine = r * G + c;
        if ((i & 63) == 63) out[i - 63 + lane] = mine;
        const int slot = r >> 1, lw = ((r & 1) << 5) | c;
        // the cell's own slot: the cell is taken; left, right and the other row of the pair are pushed
        const bool take = lane == lw;
        const bool push = ((c > 0) & (lane == lw - 1)) | ((c < 31) & (lane == lw + 1)) | (lane == (lw ^ 32));
        // the row on the other side: the slot above for an even row, the slot below for an odd one (none: any slot, nothing pushed)
        const int beside = slot + ((r & 1) ? 1 : -1), slot2 = beside & 15;
        const bool push2 = (slot2 == beside) & (lane == (lw ^ 32));
        // slot and slot2 are the same in every lane: the registers are indexed through a scalar, one element read and written
        const uint32_t x = v[slot];
        v[slot] = take ? TAKEN : push ? x & ~UNSEEN : x;
        const uint32_t y = v[slot2];
        v[slot2] = push2 ? y & ~UNSEEN : y;
    }
    if (lane < (L & 63)) out[(L & ~63) + lane] = mine;
    if (lane == 0 && first_steps) first_steps[b] = first;
}

}  // namespace

extern "C" {

const char *ps_plan_last_error(void) { return ps::last_error_ref().c_str(); }

int ps_plan_order_takes(int S, int G)
{
    return G >= 1 && G <= PLAN_GMAX && S >= G && S <= PLAN_SMAX && S % G == 0;
}

int ps_plan_order(const uint8_t *bg, int B, int S, int G, int32_t *order_loc, uint8_t *region, int32_t *first_steps,
                  int32_t *bg_counts, void *stream)
{
    static_assert(CH_M1 == (uint32_t)(1.4f * 65536.0 + 0.5) && CH_M2 == (uint32_t)(2.1969f * 65536.0 + 0.5), "chamfer metrics");
    PS_REQUIRE(bg && order_loc && region, "plan_order: null pointer");
    PS_REQUIRE(B > 0, "plan_order: B must be > 0");
    PS_REQUIRE(ps_plan_order_takes(S, G), "plan_order: S = %d, G = %d is not taken (1 <= G <= %d, S a multiple of G, S <= %d)", S, G,
               PLAN_GMAX, PLAN_SMAX);
    const int vec = S % 16 == 0 && ((uintptr_t)bg & 15) == 0;
    hipLaunchKernelGGL(k_plan_order, dim3(B), dim3(PLAN_THREADS), 0, (hipStream_t)stream, bg, S, G, vec, order_loc, region,
                       first_steps, bg_counts);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
