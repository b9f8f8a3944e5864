// rank_select.h -- the rank rule of get_best_sample for ONE group of n candidates, as a workgroup runs it: the device code that
// k_rank_select (rank.hip, one group) and k_rank_select_groups (rank_groups.hip, one workgroup per group) share.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pixelsynth_rank.h"

namespace ps_rank {

constexpr int SELECT_THREADS = 256;                  // the workgroup of select_group

// a (at index j) sorts before b (at index i): ascending, the lower index first among equals, NaN after every number
__device__ __forceinline__ bool sorts_before(float a, int j, float b, int i)
{
    const bool an = a != a, bn = b != b;
    if (an || bn) return an == bn ? j < i : bn;
    return a < b || (a == b && j < i);
}

// Called by every thread of a workgroup of SELECT_THREADS.  Score i of either list lies at [i * stride], rank i is written to
// [i * stride] (disc_rank, entr_rank: or null).  Both lists in LDS, every element's rank by counting, the packed (total, index)
// maximum; best[0] = the first index of the largest total2.  1 <= n <= PS_RANK_MAX_N (the host checks it).
__device__ __forceinline__ void select_group(const float *__restrict__ disc, const float *__restrict__ entr, int n, long stride,
                                             int32_t *__restrict__ best, int32_t *__restrict__ disc_rank,
                                             int32_t *__restrict__ entr_rank)
{
    __shared__ float s_d[PS_RANK_MAX_N], s_e[PS_RANK_MAX_N];
    __shared__ uint32_t s_key[SELECT_THREADS / 64];
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += SELECT_THREADS) s_d[i] = disc[i * stride], s_e[i] = entr[i * stride];
    __syncthreads();
    uint32_t key = 0;                                // total2 << 10 | (1023 - index): its maximum is the first index of the largest total2
    for (int i = tid; i < n; i += SELECT_THREADS) {
        const float d = s_d[i], e = s_e[i];
        int dr = 0, er = 0;
        for (int j = 0; j < n; ++j) {
            dr += sorts_before(s_d[j], j, d, i);
            er += sorts_before(s_e[j], j, e, i);
        }
        if (disc_rank) disc_rank[i * stride] = dr;
        if (entr_rank) entr_rank[i * stride] = er;
        key = max(key, ((uint32_t)(n - 1 - er + dr) << 10) | (uint32_t)(PS_RANK_MAX_N - 1 - i));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, d, 64));
    if ((tid & 63) == 0) s_key[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SELECT_THREADS / 64; ++w) key = max(key, s_key[w]);
        best[0] = PS_RANK_MAX_N - 1 - (int32_t)(key & (PS_RANK_MAX_N - 1));
    }
}

}  // namespace ps_rank
