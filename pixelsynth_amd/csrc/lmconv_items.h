// lmconv_items.h -- the items of a whole-grid pass as the kernels see them: the ItemMap every product and post-op kernel of
// lmconv_grid.hip takes as an argument and the planning kernels of lmconv_plan.hip fill the tables of.  Its fields are set in
// lmconv_plan.hip alone (plan_grid); its layout is part of the compiled kernels.
#pragma once
#include "ps_common.h"

namespace pslm {

constexpr int STARTS_MAXL = 4096;   // locations of a grid whose pass can be planned (ranks held in LDS, 12-bit locations in permq)

// Items of a whole-grid pass: every (frame, location) pair, or -- with a generation order -- only the first
// `npre` locations of each frame in that order (the observed prefix an AR run starts from; later locations
// are produced by the column steps, and no earlier location ever reads them).
struct ItemMap {
    const int32_t *order;  // (F, L) location by rank, or null = all L locations in raster order
    int npre;              // locations per frame
    const int32_t *start;  // (F) or null: ranks below start[f] are NOT evaluated at this stage -- nothing reads them
                           // (k_prefix_starts); only with an order
    int f0;                // first frame of the pass (a pass over frames [f0, f0 + n): item 0 is rank 0 of frame f0)
    const int32_t *perm;   // or null: position p of the products' item list holds item perm[p] -- the items grouped by their set of
                           // open taps (k_perm_*), so that a tile of 16 / 32 items shares its taps; the post ops walk the items as they are
    const int2 *permq;     // the same list as (item, location) pairs: one load instead of the chain position -> item -> order -> location
    const int32_t *end;    // (F) or null: frame f's prefix ends at rank end[f] <= npre (per-frame prefixes: the ranks from there on are
                           // its columns'); only with an order
    const uint32_t *bits;  // (F, bw) or null: the EXACT set of ranks evaluated at this stage, one bit per rank (k_prefix_sets); takes the
    int bw;                // place of `start` (a subset of its suffix, already cut at the frame's end); bw = 32-bit words per frame
    // the stage's own item list (k_perm_compact): the entries of `permq` that are evaluated at this stage, share by share (a share = the
    // frames of one XCD, or all of them: cparts = 8 / 1), in the order permq has them; share s starts at cq[s * cshare] and holds
    // ccnt[s] entries.  Read by k_gemm_ws; every other kernel walks permq / the items and asks item_wanted.
    const int2 *cq;
    const int32_t *ccnt;
    int cshare, cparts;
};
// item at position `pos` of the products' item list, -1 past its end
__device__ __forceinline__ int item_at(const ItemMap &m, int pos, int nitems)
{
    if (pos >= nitems) return -1;
    return m.perm ? m.perm[pos] : pos;
}
__device__ __forceinline__ void item_loc(const ItemMap &m, int item, int L, int &f, int &q)
{
    const int fl = item / m.npre;
    const int r = item - fl * m.npre;
    f = m.f0 + fl;
    q = m.order ? m.order[(size_t)f * L + r] : r;
}
// is the item evaluated at this stage?
__device__ __forceinline__ bool item_wanted(const ItemMap &m, int item)
{
    if (!m.start && !m.end && !m.bits) return true;
    const int fl = item / m.npre, r = item - fl * m.npre;
    if (m.bits) return (m.bits[(size_t)(m.f0 + fl) * m.bw + (r >> 5)] >> (r & 31)) & 1u;   // (no bit at or behind the frame's end)
    return (!m.start || r >= m.start[m.f0 + fl]) && (!m.end || r < m.end[m.f0 + fl]);
}

}  // namespace pslm
