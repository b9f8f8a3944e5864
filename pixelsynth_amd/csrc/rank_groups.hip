// rank_groups.hip -- best-of-N PER VIEW for a batch of views, for gfx950 (MI355X): the rank rule of get_best_sample applied to every
// view's own candidates, and the hand-over of every view's winner, both on the device.
//
// Behind the C ABI of include/pixelsynth_rank_groups.h (libpixelsynth_rank_groups.so, beside libpixelsynth_rank.so whose set of exports
// it leaves as it is).  Two passes, no atomic, nothing summed:
//   k_rank_select_groups  one workgroup per group (view): rank_select.h's select_group -- the code of k_rank_select -- on the group's
//                         scores, which lie `cand_stride` apart.
//   k_rank_take_groups    grid (chunks of an item, groups): every workgroup reads its group's winner index, clamps it into 0 .. n-1 and
//                         copies one chunk of that item, 16 bytes per lane where the host found the addresses aligned.
#include "ps_common.h"

#include "../../include/pixelsynth_rank_groups.h"
#include "rank_select.h"

namespace {

constexpr int TAKE_THREADS = 256;
constexpr int TAKE_CHUNK = 4096;                     // floats of an item per workgroup: four float4 (or sixteen floats) per thread

__global__ __launch_bounds__(ps_rank::SELECT_THREADS) void k_rank_select_groups(const float *__restrict__ disc,
                                                                                const float *__restrict__ entr, int n,
                                                                                long group_stride, long cand_stride,
                                                                                int32_t *__restrict__ best,
                                                                                int32_t *__restrict__ disc_rank,
                                                                                int32_t *__restrict__ entr_rank)
{
    const long base = (long)blockIdx.x * group_stride;
    ps_rank::select_group(disc + base, entr + base, n, cand_stride, best + blockIdx.x, disc_rank ? disc_rank + base : nullptr,
                          entr_rank ? entr_rank + base : nullptr);
}

template <typename T>   // T = float4: item_len counts float4s, src and out are 16-byte aligned; T = float: any
__device__ __forceinline__ void take_chunk(const T *__restrict__ src, T *__restrict__ out, long item_len, long first)
{
    constexpr int PER_THREAD = TAKE_CHUNK * (int)sizeof(float) / (int)sizeof(T) / TAKE_THREADS;
    T v[PER_THREAD];                                 // every load of the thread in flight before its first store
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const long i = first + (long)k * TAKE_THREADS + threadIdx.x;
        if (i < item_len) v[k] = src[i];
    }
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const long i = first + (long)k * TAKE_THREADS + threadIdx.x;
        if (i < item_len) out[i] = v[k];
    }
}

__global__ __launch_bounds__(TAKE_THREADS) void k_rank_take_groups(const float *__restrict__ src, const int32_t *__restrict__ best,
                                                                   int n, long group_stride, long cand_stride, long item_floats,
                                                                   float *__restrict__ out, int vec)
{
    const long g = blockIdx.y;
    const int b = best[g];
    const long item = g * group_stride + (long)(b < 0 ? 0 : b > n - 1 ? n - 1 : b) * cand_stride;
    const float *s = src + item * item_floats;
    float *o = out + g * item_floats;
    if (vec)
        take_chunk(reinterpret_cast<const float4 *>(s), reinterpret_cast<float4 *>(o), item_floats / 4,
                   (long)blockIdx.x * (TAKE_CHUNK / 4));
    else
        take_chunk(s, o, item_floats, (long)blockIdx.x * TAKE_CHUNK);
}

// the two layouts of n candidates of `groups` groups: candidate-major (1, groups), group-major (n, 1)
bool layout_ok(int groups, int n, long group_stride, long cand_stride)
{
    return (group_stride == 1 && cand_stride == groups) || (group_stride == n && cand_stride == 1);
}

}  // namespace

extern "C" {

const char *ps_rank_groups_last_error(void) { return ps::last_error_ref().c_str(); }

int ps_rank_select_groups(const float *disc, const float *entr, int groups, int n, long group_stride, long cand_stride, int32_t *best,
                          int32_t *disc_rank, int32_t *entr_rank, void *stream)
{
    PS_REQUIRE(disc && entr && best, "rank_select_groups: null pointer");
    PS_REQUIRE(n >= 1 && n <= PS_RANK_MAX_N, "rank_select_groups: n = %d, expected 1 .. %d", n, PS_RANK_MAX_N);
    PS_REQUIRE(groups >= 1 && groups <= PS_RANK_MAX_GROUPS, "rank_select_groups: groups = %d, expected 1 .. %d", groups,
               PS_RANK_MAX_GROUPS);
    PS_REQUIRE(layout_ok(groups, n, group_stride, cand_stride),
               "rank_select_groups: strides (group %ld, candidate %ld), expected (1, %d) candidate-major or (%d, 1) group-major",
               group_stride, cand_stride, groups, n);
    hipLaunchKernelGGL(k_rank_select_groups, dim3(groups), dim3(ps_rank::SELECT_THREADS), 0, (hipStream_t)stream, disc, entr, n,
                       group_stride, cand_stride, best, disc_rank, entr_rank);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

int ps_rank_take_groups(const float *src, const int32_t *best, int groups, int n, long group_stride, long cand_stride, long item_floats,
                        float *out, void *stream)
{
    PS_REQUIRE(src && best && out, "rank_take_groups: null pointer");
    PS_REQUIRE(n >= 1 && n <= PS_RANK_MAX_N, "rank_take_groups: n = %d, expected 1 .. %d", n, PS_RANK_MAX_N);
    PS_REQUIRE(groups >= 1 && groups <= PS_RANK_MAX_GROUPS, "rank_take_groups: groups = %d, expected 1 .. %d", groups, PS_RANK_MAX_GROUPS);
    PS_REQUIRE(layout_ok(groups, n, group_stride, cand_stride),
               "rank_take_groups: strides (group %ld, candidate %ld), expected (1, %d) candidate-major or (%d, 1) group-major",
               group_stride, cand_stride, groups, n);
    const long max_item = (long)TAKE_CHUNK * 0x7fffffffL;                        // (grid.x)
    PS_REQUIRE(item_floats >= 1 && item_floats <= max_item, "rank_take_groups: item_floats = %ld, expected 1 .. %ld", item_floats, max_item);
    const int vec = item_floats % 4 == 0 && ((uintptr_t)src | (uintptr_t)out) % 16 == 0;
    const long chunks = (item_floats + TAKE_CHUNK - 1) / TAKE_CHUNK;
    hipLaunchKernelGGL(k_rank_take_groups, dim3((unsigned)chunks, groups), dim3(TAKE_THREADS), 0, (hipStream_t)stream, src, best, n,
                       group_stride, cand_stride, item_floats, out, vec);
    PS_LAUNCH_CHECK();
    return PS_OK;
}

}  // extern "C"
