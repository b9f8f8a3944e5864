// lmconv_plan.hip -- planning of a whole-grid pass of the locally-masked PixelCNN engine: WHICH items every stage evaluates (k_prefix_starts,
// k_prefix_sets) and in which order the products walk them (k_perm_*).  run_grid (lmconv_grid.hip) asks plan_grid for a GridPlan and
// takes the ItemMap of every launch from it.
#include "lmconv_handle.h"

namespace pslm {

// ------------------------------------------------------------------------------------------
// Which prefix items does anybody read?  The whole-grid pass over the observed prefix of an AR run exists for ONE reason:
// the column steps read the finished activations of earlier neighbours.  A column reads, per stage, the open taps of its
// location -- so from the prefix only a band along the frontier; those items read their own open taps one stage
// earlier, and so on backwards through the 32 stages: a dependency cone, not the whole prefix at every stage (63-83 %
// of the work for PixelSynth's orders).  Because the generation order sweeps towards the frontier, the cone
// of a stage is -- up to a few items -- a SUFFIX of the prefix in rank order, so it is kept as one number per (stage,
// frame): the smallest rank anyone reads; items of lower rank are skipped at that stage (their cache rows keep whatever
// they held; nothing reads them).  The taps come from the kernel masks themselves, exactly what the kernels follow.
// One workgroup per frame; starts[(stage id) * F + f] with the evaluation-stage ids of lmconv_device.h (eval_conv_in, eval_conv_out,
// eval_dil; 0 = u_init).
// ------------------------------------------------------------------------------------------
struct StartsArgs {
    const int32_t *order;   // (F, L)
    const float *mask_und, *mask_dil;   // (F, 9, L): type B dilation 1 / dilation 2
    int H, W, L, npre, F;
    int32_t *starts;        // (N_EVAL, F)
    int f0;                 // frames [f0, f0 + gridDim.x) of the F
    const int32_t *pend;    // (F) or null: the prefix of frame f is its ranks [0, pend[f]) instead of [0, npre)
};
__global__ __launch_bounds__(1024) void k_prefix_starts(StartsArgs a)
{
    __shared__ int rank[STARTS_MAXL];   // by location
    __shared__ int s1[STARTS_MAXL];     // by rank < npre: min rank among the open dilation-1 taps of ranks >= r (suffix minimum)
    __shared__ int s2[STARTS_MAXL];     //                 the same, dilation-2 taps of the dilated mask
    __shared__ int cmin[2];             // min rank the COLUMNS (ranks >= npre) read through dilation-1 / dilation-2 taps
    const int f = a.f0 + blockIdx.x, t = threadIdx.x, L = a.L, npre = a.pend ? a.pend[f] : a.npre;
    const int32_t *ord = a.order + (size_t)f * L;
    for (int r = t; r < L; r += 1024) rank[ord[r]] = r;
    if (t < 2) cmin[t] = npre;
    __syncthreads();
    for (int r = t; r < L; r += 1024) {
        const int q = ord[r], y = q / a.W, x = q - y * a.W;
        int m1 = npre, m2 = npre;
        for (int tap = 0; tap < 9; ++tap) {
            if (tap == 4) continue;
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            if (a.mask_und[((size_t)f * 9 + tap) * L + q] != 0.0f) {
                const int yy = y + dy, xx = x + dx;
                if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) m1 = min(m1, rank[yy * a.W + xx]);
            }
            if (a.mask_dil[((size_t)f * 9 + tap) * L + q] != 0.0f) {
                const int yy = y + 2 * dy, xx = x + 2 * dx;
                if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) m2 = min(m2, rank[yy * a.W + xx]);
            }
        }
        if (r < npre) { s1[r] = m1; s2[r] = m2; }
        else { atomicMin(&cmin[0], m1); atomicMin(&cmin[1], m2); }
    }
    __syncthreads();
    for (int off = 1; off < npre; off <<= 1) {   // suffix minima by doubling
        int v1[STARTS_MAXL / 1024], v2[STARTS_MAXL / 1024];
#pragma unroll
        for (int k = 0; k < STARTS_MAXL / 1024; ++k) {
            const int r = t + 1024 * k;
            if (r < npre) {
                v1[k] = r + off < npre ? min(s1[r], s1[r + off]) : s1[r];
                v2[k] = r + off < npre ? min(s2[r], s2[r + off]) : s2[r];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < STARTS_MAXL / 1024; ++k) {
            const int r = t + 1024 * k;
            if (r < npre) { s1[r] = v1[k]; s2[r] = v2[k]; }
        }
        __syncthreads();
    }
    if (t != 0) return;
    auto suf = [&](const int *s, int r0) { return r0 >= npre ? npre : min(r0, s[r0]); };   // ranks [r0, npre) and all they read
    constexpr StageGraph sg = stage_graph();
    int need[NNODE], needX[NGATED];
    for (int n = 0; n < NNODE; ++n) need[n] = npre;
    for (int g = 0; g < NGATED; ++g) { needX[g] = cmin[0]; need[sg.g_in[g]] = min(need[sg.g_in[g]], cmin[0]); }
    for (int d = 0; d < NDIL; ++d) need[sg.d_in[d]] = min(need[sg.d_in[d]], cmin[1]);
    // backwards through the blocks in execution order
    int32_t *out = a.starts + f;
    for (int e = NBLOCK - 1; e >= 0; --e) {
        if (sg.order[e] < NGATED) {
            const int g = sg.order[e];
            const int so = need[sg.g_out[g]];                     // conv_out + gate evaluated from rank so on
            out[(size_t)eval_conv_out(g) * a.F] = so;
            needX[g] = min(needX[g], suf(s1, so));               //   reads conv_input's output at its open taps
            need[sg.g_in[g]] = min(need[sg.g_in[g]], so);          //   and the residual input at the same location
            const int si = needX[g];                             // conv_input (+ nin_skip) evaluated from rank si on
            out[(size_t)eval_conv_in(g) * a.F] = si;
            need[sg.g_in[g]] = min(need[sg.g_in[g]], suf(s1, si));
            if (sg.g_skip[g] >= 0) need[sg.g_skip[g]] = min(need[sg.g_skip[g]], si);
        } else {
            const int d = sg.order[e] - NGATED;
            const int sd = need[sg.d_out[d]];
            out[(size_t)eval_dil(d) * a.F] = sd;
            need[sg.d_in[d]] = min(need[sg.d_in[d]], suf(s2, sd));
        }
    }
    out[0] = need[0];   // u_init + norm_init
}

// ------------------------------------------------------------------------------------------
// The same cone as EXACT sets (tune.prefix_exact).  The suffix form evaluates every rank from the smallest one anybody reads; with the
// whole-grid pass the largest phase of a step, the ranks inside that suffix that nobody reads (11-12 % of the items of PixelSynth's
// orders) are worth leaving out too.  One workgroup per frame walks the stages backwards exactly as k_prefix_starts does, with one bit
// per rank in LDS instead of one number: the set a stage evaluates, the ranks those read through their open taps one stage earlier
// (plus themselves, for the residual input), and so on; everything is cut at the frame's own end.  The numpy restatement is
// exact_need_sets (oracle/prefix_cone_oracle.py).  bits[(stage id * F + f) * bw + w], stage ids as above.
// A thread owns ranks t, t + 1024, ... and keeps the ranks of their open, in-grid, in-prefix neighbours in registers (two per dword,
// 0xFFFF = none), so a step of the walk is LDS traffic only.  K = ranks per thread: 1 for grids of up to 1024 locations, 2, 4.
// ------------------------------------------------------------------------------------------
constexpr int SETS_W = STARTS_MAXL / 32;
template <int K>
__global__ __launch_bounds__(1024) void k_prefix_sets(StartsArgs a, uint32_t *bits, int bw)
{
    __shared__ unsigned short rank[STARTS_MAXL];   // by location
    __shared__ uint32_t need[NNODE][SETS_W];       // ranks of node n's activations that somebody reads
    __shared__ uint32_t needX[NGATED][SETS_W];     // the same for the output of conv_input inside gated block g
    __shared__ uint32_t col[2][SETS_W];            // what the COLUMNS (ranks >= npre) read through dilation-1 / dilation-2 taps
    const int f = a.f0 + blockIdx.x, t = threadIdx.x, L = a.L, npre = a.pend ? a.pend[f] : a.npre;
    const int32_t *ord = a.order + (size_t)f * L;
    for (int r = t; r < L; r += 1024) rank[ord[r]] = (unsigned short)r;
    for (int w = t; w < NNODE * SETS_W; w += 1024) (&need[0][0])[w] = 0u;
    for (int w = t; w < NGATED * SETS_W; w += 1024) (&needX[0][0])[w] = 0u;
    for (int w = t; w < 2 * SETS_W; w += 1024) (&col[0][0])[w] = 0u;
    __syncthreads();
    auto set_bit = [](uint32_t *s, int r) { atomicOr(&s[r >> 5], 1u << (r & 31)); };
    uint32_t nb[2][K][4];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int r = t + 1024 * k;
#pragma unroll
        for (int kind = 0; kind < 2; ++kind)
#pragma unroll
            for (int n = 0; n < 4; ++n) nb[kind][k][n] = 0xFFFFFFFFu;
        if (r >= L) continue;
        const int q = ord[r], y = q / a.W, x = q - y * a.W;
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int tap = n < 4 ? n : n + 1, dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
            for (int kind = 0; kind < 2; ++kind) {
                const float *mask = kind == 0 ? a.mask_und : a.mask_dil;
                const int yy = y + (kind + 1) * dy, xx = x + (kind + 1) * dx;
                if (mask[((size_t)f * 9 + tap) * L + q] == 0.0f || yy < 0 || yy >= a.H || xx < 0 || xx >= a.W) continue;
                const int nr = rank[yy * a.W + xx];
                if (nr >= npre) continue;                       // (a column's activations are the column steps' business)
                if (r >= npre) set_bit(col[kind], nr);
                else nb[kind][k][n >> 1] = (n & 1) ? (nb[kind][k][n >> 1] & 0x0000FFFFu) | (uint32_t)nr << 16 : (nb[kind][k][n >> 1] & 0xFFFF0000u) | (uint32_t)nr;
            }
        }
    }
    __syncthreads();
    // dst |= the prefix ranks of `src` and the prefix ranks they read through the open taps of mask kind `kind` (src != dst)
    auto reads = [&](const uint32_t *src, uint32_t *dst, int kind) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int r = t + 1024 * k;
            if (r >= npre || !((src[r >> 5] >> (r & 31)) & 1u)) continue;
            set_bit(dst, r);
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                const uint32_t pair = kind == 0 ? nb[0][k][n >> 1] : nb[1][k][n >> 1];
                const int nr = (int)((n & 1) ? pair >> 16 : pair & 0xFFFFu);
                if (nr != 0xFFFF) set_bit(dst, nr);
            }
        }
        __syncthreads();
    };
    auto join = [&](uint32_t *dst, const uint32_t *src) {      // dst |= src
        for (int w = t; w < bw; w += 1024) dst[w] |= src[w];
        __syncthreads();
    };
    auto emit = [&](int stage, const uint32_t *src) {
        for (int w = t; w < bw; w += 1024) bits[((size_t)stage * a.F + f) * bw + w] = src[w];
    };
    constexpr StageGraph sg = stage_graph();
    for (int g = 0; g < NGATED; ++g) { join(needX[g], col[0]); join(need[sg.g_in[g]], col[0]); }
    for (int d = 0; d < NDIL; ++d) join(need[sg.d_in[d]], col[1]);
    for (int e = NBLOCK - 1; e >= 0; --e) {
        if (sg.order[e] < NGATED) {
            const int g = sg.order[e];
            const uint32_t *so = need[sg.g_out[g]];               // conv_out + gate
            emit(eval_conv_out(g), so);
            reads(so, needX[g], 0);                              //   reads conv_input's output at its open taps
            join(need[sg.g_in[g]], so);                           //   and the residual input at the same location
            const uint32_t *si = needX[g];                       // conv_input (+ nin_skip)
            emit(eval_conv_in(g), si);
            reads(si, need[sg.g_in[g]], 0);
            if (sg.g_skip[g] >= 0) join(need[sg.g_skip[g]], si);
        } else {
            const int d = sg.order[e] - NGATED;
            const uint32_t *sd = need[sg.d_out[d]];
            emit(eval_dil(d), sd);
            reads(sd, need[sg.d_in[d]], 1);
        }
    }
    emit(0, need[0]);   // u_init + norm_init
}

// ------------------------------------------------------------------------------------------
// Items grouped by their set of open taps (round 5).  A tile of the products computes a tap for all its items as soon as ONE of
// them has it open; a location has 4.7 of its 9 taps open on average (of every adjacent pair exactly one precedes the other), a
// tile of 16 consecutive ranks of a frame 7.1 of 9, a tile of 32 already 8.1 -- a third of the MFMA work of the pass multiplied
// zeros.  The masks of a frame take about 40 distinct tap sets, so the items are SORTED by tap set (9 bits: tap t open and inside
// the grid) and the products walk that list: 4.8 taps per tile of 16, 4.85 per tile of 32.  A closed tap adds an exact zero, so
// which items share a tile changes no bit; the post ops and every cache row are addressed by the item itself, as before.
// Order inside a tap set: frame, then rank (neighbouring ranks are neighbouring locations: their input rows are the same lines).
// `nparts` > 1: one sort per share of the frames, so that the contiguous range of tiles an XCD takes (k_gemm / k_gemm_wg) reads
// the rows of ITS frames only.  Three small launches per pass and mask kind (dilation 1, dilation 2):
//   k_perm_sort     per frame: (tap set's place << 13 | rank << 1 | fractional masks) of its items, sorted (bitonic, LDS), and the run
//                   length of every tap set
//   k_perm_scan     first position of every (share, tap set, frame) run: exclusive scan over [share][tap set][frame], in tiles of
//                   1024 entries (the tiles' totals are scanned by every block of the next launch for itself)
//   k_perm_scatter  per frame: perm[first + index in the run] = item
// ------------------------------------------------------------------------------------------
struct PermArgs {
    const int32_t *order;               // (F, L) or null (raster)
    const float *mask[2];               // (F, 9, L): type B dilation 1 / dilation 2
    int H, W, L, npre, f0, nf, nparts;
    uint32_t *sorted[2];                // [nf][npre]
    int32_t *cnt[2];                    // [nparts][512][frames per share]
    int32_t *tsum[2];                   // totals of the table's tiles of 1024 entries
    int32_t *perm[2];                   // [nf * npre]
    int2 *permq[2];                     // the same as (item, location) pairs
    const int32_t *pend;                // (F) or null: ranks >= pend[f] of frame f are not part of its prefix (they sort behind everything)
};
constexpr int PERM_KEYS = 512;
// Sort key of a tap set: its place in the order (number of open taps, descending; then the 9-bit set).  The workgroups of a launch
// are dispatched in item order, so the tiles with the most taps -- the longest jobs -- start first and the launch's tail is made of
// the cheapest ones (longest-processing-time-first: a tile of 7 open taps costs twice one of 3, and 64-item workgroups fill the
// chip only two to three times over).
struct PermBins { unsigned short v[PERM_KEYS]; };
constexpr PermBins make_perm_bins()
{
    PermBins t{};
    int n = 0;
    for (int pc = 9; pc >= 0; --pc)
        for (int p = 0; p < PERM_KEYS; ++p)
            if (__builtin_popcount((unsigned)p) == pc) t.v[p] = (unsigned short)n++;
    return t;
}
__device__ const PermBins g_perm_bin = make_perm_bins();
constexpr PermBins make_perm_pats()   // the inverse: place -> tap set
{
    PermBins t{}, b = make_perm_bins();
    for (int p = 0; p < PERM_KEYS; ++p) t.v[b.v[p]] = (unsigned short)p;
    return t;
}
__device__ const PermBins g_perm_pat = make_perm_pats();
__device__ __forceinline__ int perm_fpp(const PermArgs &a) { return (a.nf + a.nparts - 1) / a.nparts; }   // frames per share
__device__ __forceinline__ size_t perm_cnt_index(const PermArgs &a, int fl, int key)
{
    const int fpp = perm_fpp(a), part = fl / fpp;
    return ((size_t)part * PERM_KEYS + key) * fpp + (fl - part * fpp);
}
__global__ __launch_bounds__(1024) void k_perm_sort(PermArgs a)
{
    __shared__ uint32_t s[STARTS_MAXL];
    __shared__ int hist[PERM_KEYS];
    const int fl = blockIdx.x, kind = blockIdx.y, f = a.f0 + fl, t = threadIdx.x, dil = kind + 1;
    const float *mask = a.mask[kind];
    int P = 2;
    while (P < a.npre) P <<= 1;
    for (int r = t; r < P; r += 1024) {
        uint32_t v = 0xFFFFFFFFu;
        if (r < a.npre) {
            const int q = a.order ? a.order[(size_t)f * a.L + r] : r, y = q / a.W, x = q - y * a.W;
            uint32_t key = 0, frac = 0;   // frac: a mask value that is neither 0 nor 1 (the reference's never are): the products load them
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int yy = y + (tap / 3 - 1) * dil, xx = x + (tap % 3 - 1) * dil;
                if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
                    const float mvv = mask[((size_t)f * 9 + tap) * a.L + q];
                    if (mvv != 0.0f) key |= 1u << tap;
                    if (mvv != 0.0f && mvv != 1.0f) frac = 1;
                }
            }
#ifdef PS_PERM_PLAIN_BINS   // (tuning builds: the tap sets in the order of their 9-bit value)
            v = key << 13 | (uint32_t)r << 1 | frac;
#else
            v = (uint32_t)g_perm_bin.v[key] << 13 | (uint32_t)r << 1 | frac;
#endif
            // (per-frame prefixes: the ranks behind a frame's own end keep their place in the item space -- nobody evaluates them,
            // item_wanted -- and are put together behind every tap set, so that they fill whole tiles, which leave at once)
            if (a.pend && r >= a.pend[f]) v = (uint32_t)(PERM_KEYS - 1) << 13 | (uint32_t)r << 1;
        }
        s[r] = v;
    }
    for (int k = t; k < PERM_KEYS; k += 1024) hist[k] = 0;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += 1024) {
                const int l = i ^ j;
                if (l > i) {
                    const uint32_t x = s[i], y = s[l];
                    if ((x > y) == ((i & k) == 0)) { s[i] = y; s[l] = x; }
                }
            }
            __syncthreads();
        }
    for (int i = t; i < a.npre; i += 1024) {
        a.sorted[kind][(size_t)fl * a.npre + i] = s[i];
        atomicAdd(&hist[s[i] >> 13], 1);
    }
    __syncthreads();
    for (int k = t; k < PERM_KEYS; k += 1024) a.cnt[kind][perm_cnt_index(a, fl, k)] = hist[k];
}
// block-wide exclusive scan of one value per thread (1024 threads); returns the exclusive prefix, *total = the block's sum
__device__ __forceinline__ int block_exscan_1024(int v, int *sh /*[1024]*/, int *total)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int u = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += u;
        __syncthreads();
    }
    *total = sh[1023];
    return sh[t] - v;
}
// grid (tiles of 1024 table entries, mask kinds): run lengths -> exclusive prefix inside the tile, + the tile's total
__global__ __launch_bounds__(1024) void k_perm_scan(PermArgs a)
{
    __shared__ int sh[1024];
    const int kind = blockIdx.y, i = blockIdx.x * 1024 + threadIdx.x;
    const int n = a.nparts * PERM_KEYS * perm_fpp(a);
    int32_t *c = a.cnt[kind];
    int total;
    const int ex = block_exscan_1024(i < n ? c[i] : 0, sh, &total);
    if (i < n) c[i] = ex;
    if (threadIdx.x == 0) a.tsum[kind][blockIdx.x] = total;
}
__global__ __launch_bounds__(1024) void k_perm_scatter(PermArgs a)
{
    __shared__ int first[PERM_KEYS];
    __shared__ int sh[1024];
    __shared__ int tbase[1024];          // first position of every tile of the run-length table (its tiles' totals, scanned)
    const int fl = blockIdx.x, kind = blockIdx.y, t = threadIdx.x;
    const int ntiles = (a.nparts * PERM_KEYS * perm_fpp(a) + 1023) / 1024;   // <= 1024: maxF <= 2048 (checked by the caller)
    int total;
    tbase[t] = block_exscan_1024(t < ntiles ? a.tsum[kind][t] : 0, sh, &total);
    const uint32_t *s = a.sorted[kind] + (size_t)fl * a.npre;
    for (int i = t; i < a.npre; i += 1024) {
        const uint32_t key = s[i] >> 13;
        if (i == 0 || (s[i - 1] >> 13) != key) first[key] = i;
    }
    __syncthreads();
    for (int i = t; i < a.npre; i += 1024) {
        const uint32_t v = s[i], key = v >> 13;
        const size_t e = perm_cnt_index(a, fl, (int)key);
        const int r = (int)((v >> 1) & 4095u), pos = a.cnt[kind][e] + tbase[e >> 10] + i - first[key];
        const int q = a.order ? a.order[(size_t)(a.f0 + fl) * a.L + r] : r;
#ifdef PS_PERM_PLAIN_BINS
        const int pat = (int)key;
#else
        const int pat = g_perm_pat.v[key];
#endif
        a.perm[kind][pos] = fl * a.npre + r;
        a.permq[kind][pos] = int2{fl * a.npre + r, q | pat << 12 | (int)(v & 1u) << 21};   // (item, location | tap set | fractional masks)
    }
}

// ------------------------------------------------------------------------------------------
// The stages' own item lists.  The sorted list holds every position of the prefix, and since the sort the ranks a stage skips sit at
// the head of every (tap set, frame) run -- spread through tiles that run anyway, at the full price of a workgroup (its set-up, its
// chunks and barriers, its post op do not depend on how many of its 64 items are evaluated).  So every (stage, share) gets a list of
// its evaluated entries alone: grid (32 product stages, shares), a workgroup walks its share's run of `permq` in order and keeps what
// item_wanted keeps -- order inside a share unchanged (tap sets heaviest first, frame, rank), shares kept apart (an XCD's tiles read
// its own frames' rows only).  out[(stage - 1) * stride + share * share_len ...], cnt[(stage - 1) * cnt_stride + share].
// ------------------------------------------------------------------------------------------
struct CompactArgs {
    ItemMap items;              // npre, f0, end of the pass
    const int2 *permq[2];       // the sorted lists (dilation 1 / dilation 2)
    const int32_t *start;       // (N_EVAL, F) or null
    const uint32_t *bits;       // (N_EVAL, F, bw) or null
    int F, bw, nitems, share_len;
    int2 *out;
    size_t stride;
    int32_t *cnt;
    int cnt_stride;
};
__global__ __launch_bounds__(1024) void k_perm_compact(CompactArgs a)
{
    __shared__ int wsum[16];
    const int stage = 1 + blockIdx.x, share = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    ItemMap m = a.items;
    m.start = a.start ? a.start + (size_t)stage * a.F : nullptr;
    m.bits = a.bits ? a.bits + (size_t)stage * a.F * a.bw : nullptr;
    m.bw = a.bw;
    const int2 *in = a.permq[eval_mask_kind(stage)];
    const int base = share * a.share_len, end = min(base + a.share_len, a.nitems);
    int2 *out = a.out + (size_t)(stage - 1) * a.stride + base;
    int kept = 0;
    for (int p0 = base; p0 < end; p0 += 1024) {
        const int p = p0 + t;
        int2 v = int2{-1, 0};
        if (p < end) v = in[p];
        const bool w = v.x >= 0 && item_wanted(m, v.x);
        const unsigned long long b = __ballot(w);
        if (lane == 0) wsum[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < 16; ++k) { before += k < wave ? wsum[k] : 0; total += wsum[k]; }
        if (w) out[kept + before + __popcll(b & ((1ull << lane) - 1ull))] = v;
        kept += total;
        __syncthreads();
    }
    if (t == 0) a.cnt[(size_t)(stage - 1) * a.cnt_stride + share] = kept;
}

// ---- host side: the tables, the launches of one pass, the ItemMap of every stage ----
int plan_scratch_alloc(ps_pixelcnn *h)
{
    PlanScratch &s = h->plan;
    const size_t frames = (size_t)h->maxF, locs = frames * h->L;
    int rc = PS_OK;
    if ((rc = dev_alloc(h, &s.pstart, N_EVAL * frames))) return rc;
    if ((rc = dev_alloc(h, &s.perm, 2 * locs))) return rc;
    if ((rc = dev_alloc(h, &s.permq, 2 * locs))) return rc;
    if ((rc = dev_alloc(h, &s.perm_sorted, 2 * locs))) return rc;
    if ((rc = dev_alloc(h, &s.perm_cnt, 2 * PERM_KEYS * frames))) return rc;
    if ((rc = dev_alloc(h, &s.perm_tsum, 2 * frames))) return rc;
    // the exact cone and the stages' own item lists: 33 x 128 B and 32 x 8 KB per frame of a 32 x 32 grid (34 MB at 128 frames)
    if ((rc = dev_alloc(h, &s.pbits, N_EVAL * frames * ((h->L + 31) / 32)))) return rc;
    if ((rc = dev_alloc(h, &s.cperm, (N_EVAL - 1) * locs))) return rc;
    return dev_alloc(h, &s.cperm_cnt, (N_EVAL - 1) * frames);
}

ItemMap all_locations(int L) { return ItemMap{nullptr, L, nullptr, 0}; }

GridPlan plan_grid(ps_pixelcnn *h, int F, const Masks &m, const int32_t *order, int npre, int f0, int nf, const int32_t *pend,
                   bool want_logits, hipStream_t st)
{
    const PlanScratch &s = h->plan;
    if (nf < 0) nf = F;
    if (!order) pend = nullptr;
    GridPlan p{};
    p.all = ItemMap{order, order ? npre : h->L, nullptr, f0};
    p.all.end = pend;
    p.nitems = nf * p.all.npre;
    p.F = F;
    p.all.bw = (h->L + 31) / 32;
    if (p.nitems <= 0) return p;  // an AR run that starts at rank 0 has no prefix
    // the prefix of an AR run: only the items somebody reads, stage by stage (k_prefix_starts).  tune.prefix_full: all of them.
    // (with out_logits the caller also gets the logits of the prefix locations: every item is needed then.  tune.prefix_cone_force
    // keeps the elimination on for the parity test, which compares the logits of the WALKED locations only.)
    const bool cone = order && (!want_logits || h->tune.prefix_cone_force) && h->L <= STARTS_MAXL && !h->tune.prefix_full;
    const bool exact = cone && h->tune.prefix_exact;    // the cone as exact sets (k_prefix_sets) instead of one start rank per stage
    if (cone) {
        StartsArgs sa{order, m.und, m.dil, h->H, h->W, h->L, npre, F, s.pstart, f0, pend};
        hipLaunchKernelGGL(k_prefix_starts, dim3(nf), dim3(1024), 0, st, sa);
        if (exact && h->L <= 1024) hipLaunchKernelGGL(k_prefix_sets<1>, dim3(nf), dim3(1024), 0, st, sa, s.pbits, p.all.bw);
        else if (exact && h->L <= 2048) hipLaunchKernelGGL(k_prefix_sets<2>, dim3(nf), dim3(1024), 0, st, sa, s.pbits, p.all.bw);
        else if (exact) hipLaunchKernelGGL(k_prefix_sets<4>, dim3(nf), dim3(1024), 0, st, sa, s.pbits, p.all.bw);
        p.start = exact ? nullptr : s.pstart;
        p.bits = exact ? s.pbits : nullptr;
    }
    // the products' item lists, grouped by open-tap set (one per mask kind); the frame range's own part of the scratch
    if (h->tune.item_sort && h->L <= STARTS_MAXL && p.all.npre >= 2 && nf <= 2048) {
        PermArgs pa{};
        pa.order = order; pa.mask[0] = m.und; pa.mask[1] = m.dil;
        pa.H = h->H; pa.W = h->W; pa.L = h->L; pa.npre = p.all.npre; pa.f0 = f0; pa.nf = nf; pa.pend = pend;
        pa.nparts = h->tune.item_sort == 2 && nf >= 2 * N_XCD && nf % N_XCD == 0 ? N_XCD : 1;   // (even shares only: the table is [share][tap set][frame])
        const size_t locs = (size_t)h->maxF * h->L, first = (size_t)f0 * h->L;
        for (int k = 0; k < 2; ++k) {
            pa.sorted[k] = s.perm_sorted + k * locs + first;
            p.perm[k] = pa.perm[k] = s.perm + k * locs + first;
            p.permq[k] = pa.permq[k] = s.permq + k * locs + first;
            pa.cnt[k] = s.perm_cnt + ((size_t)k * h->maxF + f0) * PERM_KEYS;
            pa.tsum[k] = s.perm_tsum + (size_t)k * h->maxF + f0;
        }
        hipLaunchKernelGGL(k_perm_sort, dim3(nf, 2), dim3(1024), 0, st, pa);
        hipLaunchKernelGGL(k_perm_scan, dim3((pa.nparts * PERM_KEYS * ((nf + pa.nparts - 1) / pa.nparts) + 1023) / 1024, 2), dim3(1024), 0, st, pa);
        hipLaunchKernelGGL(k_perm_scatter, dim3(nf, 2), dim3(1024), 0, st, pa);
        if (cone && h->tune.prefix_compact) {   // the stages' own lists of evaluated items, for k_gemm_ws
            const int cparts = pa.nparts, cshare = cparts > 1 ? (nf / cparts) * p.all.npre : p.nitems;
            p.cq = s.cperm + first; p.cq_stride = locs;
            p.ccnt = s.cperm_cnt + f0; p.ccnt_stride = (size_t)h->maxF;
            CompactArgs ca{p.all, {p.permq[0], p.permq[1]}, p.start, p.bits, F, p.all.bw, p.nitems, cshare,
                           s.cperm + first, locs, s.cperm_cnt + f0, h->maxF};
            hipLaunchKernelGGL(k_perm_compact, dim3(N_EVAL - 1, cparts), dim3(1024), 0, st, ca);
            p.all.cshare = cshare; p.all.cparts = cparts;
        }
    }
    return p;
}

ItemMap GridPlan::walk(int eval_stage) const
{
    ItemMap it = all;
    if (start) it.start = start + (size_t)eval_stage * F;
    if (bits) it.bits = bits + (size_t)eval_stage * F * all.bw;
    return it;
}

ItemMap GridPlan::products(int eval_stage) const
{
    ItemMap it = walk(eval_stage);
    const int kind = eval_mask_kind(eval_stage);
    it.perm = perm[kind];
    it.permq = permq[kind];
    const size_t n = (size_t)(eval_stage - 1);   // (the product stages are the stages from 1 on)
    if (cq) { it.cq = cq + n * cq_stride; it.ccnt = ccnt + n * ccnt_stride; }
    return it;
}

}  // namespace pslm
