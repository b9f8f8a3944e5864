"""Shared by tests/test_splat_routes_cpu.py and tests/test_splat_routes_gpu.py: a numpy mirror of the binning arithmetic of
pixelsynth_amd/csrc/splat_math.h and splat_pipeline.h, the compositing in float64 from the oracle's hit lists, and the table of cases the two tests walk.
No test in here, and nothing of the library is imported.

Why a mirror.  Which kernel, and which branch of it, a call of the splat takes is decided by integers: tiles per frame, tiles per
point, keys per tile list.  bins() recomputes them from the points with the kernel's own fp32 operations in the kernel's order, so that
the CPU test can ASSERT that a case reaches the branch it is there for ("a workgroup of 256 points holds a footprint of more than nine
tiles", "more than 128 lists of more than 512 keys") instead of hoping so, and a case cannot drift away from its branch unnoticed.

Why float64.  composite64() takes the part of the oracle's answer that integers decide and that the kernels reproduce bit for bit (idx:
which points hit a pixel, in which order; dist: their squared distances) and does everything behind it -- division, clamp, root, power,
blend -- in float64.  The product route's bar is stated against it:
    max |gpu - composite64| <= E_ref + PRODUCT_ALLOWANCE * max |feature|,     E_ref = max |oracle_fp32 - composite64|
which is the 4e-7 x max |feature| that test_splat_gpu.py grants the route's early-out, 1-ulp root and fused multiply-add against the fp32
oracle, restated against fp64 by the triangle inequality.
"""
from collections import namedtuple

import numpy as np

# --- constants of pixelsynth_amd/csrc/, restated (by name: splat_math.h's TILE, the others splat_pipeline.h's)
TILE = 8                 # TILE            pixels per tile edge
SORT_SMALL_CAP = 512     # SORT_SMALL_CAP  keys one wave sorts in registers (k_sort_small); 64 / 128 / 256 / 512 pick 1 / 2 / 4 / 8 keys per lane
SORT_BIG_CAP = 8192      # SORT_BIG_CAP    keys a workgroup of k_sort_big sorts in LDS; longer lists are sorted in global memory
LDS_TILES = 4096         # LDS_TILES       tiles per frame up to which k_bin_count / k_bin_fill aggregate in LDS
MAX_TPP = 9              # MAX_TPP         tiles per point up to which k_bin_fill keeps LDS ranks
BIN_THREADS = 256        # __launch_bounds__ of k_bin_count / k_bin_fill: points per workgroup
SCAN_THREADS = 1024      # __launch_bounds__ of k_scan: threads of its one workgroup per frame, (NT + 1023) / 1024 counters each
SORT_BIG_WGS = 128       # splat_core's launch of k_sort_big: its workgroups, grid-striding over the worklist
DB_MAXW = 2048 // 64     # DB_MAXW         words per row of k_dilate_bits (splat_core takes it for sizes that are a multiple of 64)
SORT_REG_CAPS = (64, 128, 256, SORT_SMALL_CAP)

# --- tolerances (none of them measured on the kernels under test)
ORACLE_VS_F64 = 2e-6         # the oracle's fp32 features against composite64, x max |feature|: the reference is usable
PRODUCT_ALLOWANCE = 4e-7     # x max |feature|, beside E_ref: tests/test_splat_gpu.py, test_product_route_stops_a_walk_...

Bins = namedtuple("Bins", "tilesX NT hw max_tiles_pp counts foot")


def plan_hw(radius_px):
    """SplatGeom's hw (splat_math.h), which make_plan takes: the half width in pixels of the conservative box of a disc"""
    return np.float32(radius_px * 1.0001 + 0.01)


def plan_max_tiles_pp(radius_px):
    """SplatGeom's max_tiles_pp (splat_math.h), which make_plan takes: the slots per point of the key array"""
    span_px = int(2.0 * float(plan_hw(radius_px))) + 2
    span_t = (span_px + TILE - 2) // TILE + 1
    return span_t * span_t


def _axis_range(p, S, hw):
    """splat_math.h's axis_range on an array of coordinates: (ok, lo_px, hi_px), fp32 throughout"""
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        c = ((p + f(1.0)) * f(S) - f(1.0)) * f(0.5)
        lo, hi = c - hw, c + hw
        ok = (hi >= f(0.0)) & (lo <= f(S - 1))          # (false for NaN / inf, like !(..) || !(..))
        lo = np.where(ok, np.maximum(lo, f(0.0)), f(0.0))
        hi = np.where(ok, np.minimum(hi, f(S - 1)), f(0.0))
        ilo, ihi = np.ceil(lo).astype(np.int64), np.floor(hi).astype(np.int64)
    ok &= ilo <= ihi
    return ok, S - 1 - ihi, S - 1 - ilo


def bins(pts, S, radius_px):
    """pts (B,N,3) float32 AS THE CALLER HANDS THEM to the splat; the kernels bin them with x and y negated (splat.hip's k_negate_xy), and so
    does this.  Returns Bins: tilesX, NT, hw, max_tiles_pp as make_plan has them, counts (B,NT) the length of every tile list, foot (B,N)
    the tiles each point's box covers (0: culled) -- splat_math.h's point_bbox and the tile loop of splat_pipeline.h's k_bin_count."""
    pts = np.asarray(pts, np.float32)
    B, N, _ = pts.shape
    tilesX = (S + TILE - 1) // TILE
    NT = tilesX * tilesX
    hw = plan_hw(radius_px)
    okx, x0, x1 = _axis_range(-pts[..., 0], S, hw)
    oky, y0, y1 = _axis_range(-pts[..., 1], S, hw)
    with np.errstate(invalid="ignore"):
        live = (pts[..., 2] >= np.float32(0.0)) & okx & oky
    tx0, tx1, ty0, ty1 = x0 // TILE, x1 // TILE, y0 // TILE, y1 // TILE
    foot = np.where(live, (tx1 - tx0 + 1) * (ty1 - ty0 + 1), 0)
    counts = np.zeros((B, NT), np.int64)
    for b in range(B):
        m = live[b]
        d = np.zeros((tilesX + 1, tilesX + 1), np.int64)      # a box adds 1 to every tile it covers: corners, then two running sums
        np.add.at(d, (ty0[b][m], tx0[b][m]), 1)
        np.add.at(d, (ty0[b][m], tx1[b][m] + 1), -1)
        np.add.at(d, (ty1[b][m] + 1, tx0[b][m]), -1)
        np.add.at(d, (ty1[b][m] + 1, tx1[b][m] + 1), 1)
        counts[b] = d.cumsum(0).cumsum(1)[:tilesX, :tilesX].reshape(-1)
    assert counts.sum() == foot.sum()
    return Bins(tilesX, NT, hw, plan_max_tiles_pp(radius_px), counts, foot)


def fill_workgroups(b):
    """Per workgroup of k_bin_fill (256 consecutive points of a cloud): does it take the direct path (k_bin_fill's `fits` / `agg`)?  (B, ceil(N/256))"""
    B, N = b.foot.shape
    pad = (-N) % BIN_THREADS
    big = np.pad(b.foot > MAX_TPP, ((0, 0), (0, pad))).reshape(B, -1, BIN_THREADS).any(-1)
    return big | (b.NT > LDS_TILES)


def denom64(S, radius_px, rad_pow):
    """pow(radius, rad_pow) as SplatGeom (splat_math.h: denom) and the oracle round it: double, then float"""
    radius = radius_px / float(S) * 2.0
    return np.float64(np.float32(radius ** rad_pow))


def recip_route(S, radius_px, rad_pow):
    """SplatGeom's pow2 (splat_math.h): the kernels multiply by 1 / denom instead of dividing (RECIP)"""
    return float(np.frexp(np.float32(denom64(S, radius_px, rad_pow)))[0]) == 0.5


def composite64(ref, feat, S, radius_px, rad_pow, tau, accumulation):
    """The compositing in float64 from the oracle's idx and dist (B,S,S,K) and feat (B,C,N) -> (B,C,S,S) float64:
    alpha = (1 - sqrt(clip(dist / denom, 1e-3f, 1))) ** tau, then ps_oracle_composite's three accumulations."""
    idx, dist = ref["idx"], ref["dist"]
    feat = np.asarray(feat)
    B, C, N = feat.shape
    hit = idx >= 0
    d = np.clip(dist.astype(np.float64) / denom64(S, radius_px, rad_pow), np.float64(np.float32(1e-3)), 1.0)
    a = np.where(hit, (1.0 - np.sqrt(d)) ** float(tau), 0.0)
    if accumulation == "alphacomposite":
        w = a * np.concatenate([np.ones_like(a[..., :1]), np.cumprod(1.0 - a, axis=-1)[..., :-1]], axis=-1)
    elif accumulation == "wsum":
        w = a
    elif accumulation == "wsumnorm":
        w = a / np.maximum(a.sum(-1, keepdims=True), np.float64(np.float32(1e-4)))
    else:
        raise KeyError(accumulation)
    n = np.where(hit, idx % N, 0)
    out = np.empty((B, C, S, S), np.float64)
    for b in range(B):
        for c in range(C):
            out[b, c] = (w[b] * feat[b, c].astype(np.float64)[n[b]]).sum(-1)
    return out


# ------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------
# route: "debug" (return_debug=True: idx / zbuf / dist / bg / negated points bit-exact, features at debug_tol), "product" (bg bit-exact,
#        features at the product bar) or "both".
# branch: the predicate tests/test_splat_routes_cpu.py asserts with bins() (BRANCHES there), args its parameter.
# mask:  "mean" -- 0.005 < bg.mean() < 0.995; "both" -- hit and missed pixels both exist; None -- the case is not about the mask.
# kcap:  the case is about the K cap: some pixels have K hits.
Case = namedtuple("Case", "id S N K r B C tau rad_pow acc ksize route branch arg cloud seed spread zlo scale holes mask kcap")


def _case(id, S, N, K, r, B=2, C=3, tau=1.0, rad_pow=2, acc="alphacomposite", ksize=13, route="debug", branch=None, arg=None,
          cloud="uniform", seed=0, spread=1.1, zlo=0.1, scale=1.0, holes=0, mask=None, kcap=False):
    return Case(id, S, N, K, r, B, C, tau, rad_pow, acc, ksize, route, branch, arg, cloud, seed, spread, zlo, scale, holes, mask, kcap)


def _small_case(id, S, N, K, r, ksize=5, branch="small", spread=1.2, **kw):
    return _case(id, S, N, K, r, ksize=ksize, route="both", branch=branch, spread=spread, zlo=-0.2, holes=3, mask="both", **kw)


SORT_LENGTHS = (64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 8192, 8193)
PILE_PIXEL = (12, 4)     # (x, y) of the output pixel the sort cases pile their points on

CASES = (
    # --- binning and scan
    _case("footprint_gt9", 64, 3000, 16, 12, branch="fill_mixed", cloud="corner256", seed=101, kcap=True),
    _case("radius_limit", 128, 400, 32, 64, branch="whole_frame", seed=102, kcap=True),
    _case("scan_two_per_thread_S264", 264, 20000, 8, 4, branch="scan_per", arg=2, seed=103, holes=5, mask="mean"),
    _case("scan_two_per_thread_S260", 260, 20000, 8, 4, branch="scan_per", arg=2, seed=104, holes=5, mask="mean"),
    _case("tiles_gt_lds_S520", 520, 30000, 8, 4, branch="nt_gt_lds", seed=105, mask="mean"),
    _case("tiles_gt_lds_S576_bits", 576, 30000, 8, 3, ksize=5, branch="nt_gt_lds", seed=106, mask="mean"),
    _case("size_limit_S2048", 2048, 60000, 2, 2.5, B=1, ksize=3, route="product", branch="tile_255", seed=107, mask="mean"),
    # --- sorts
    *(_case(f"sort_len_{n}", 16, n, n, 1.5, B=1, ksize=1, branch="one_list", arg=n, cloud="pile", seed=200 + i, mask="both", kcap=True)
      for i, n in enumerate(SORT_LENGTHS)),
    _case("sort_big_second_trip", 128, 60000, 16, 4, B=1, branch="big_lists", arg=SORT_BIG_WGS, seed=220, kcap=True),
    # --- composite instantiations, both routes: small frames, some points culled (z from -0.2), a few holes in the cloud
    *(_small_case(f"{acc}_tau{tau:g}", 40, 3000, 16, 4, acc=acc, tau=tau, seed=300 + i)
      for i, (acc, tau) in enumerate((("wsum", 1.0), ("wsum", 2.0), ("wsumnorm", 1.0), ("wsumnorm", 2.0)))),
    *(_small_case(f"channels_{C}", 36, 2000, 8, 3, C=C, ksize=3, seed=310 + C, kcap=True) for C in (4, 5, 7, 8)),
    _small_case("division_S40", 40, 3000, 16, 4, branch="division", seed=320),
    _small_case("division_S40_scale50", 40, 3000, 16, 4, branch="division", seed=321, scale=50.0),
    _small_case("partial_tiles_S20", 20, 600, 8, 2.5, ksize=3, branch="partial_recip", seed=322, spread=0.6, kcap=True),
    # (tau < 1: alpha = a ** tau has an unbounded derivative at a = 0, a hit at the rim of its disc, so the fp32 oracle itself is within
    # ORACLE_VS_F64 of float64 only where no such hit lies near the front of a pixel's list: 6e-7 ... 2.6e-5 over thirty seeds.  These
    # seeds are ones where it is -- chosen on the oracle, the reference, alone.)
    *(_small_case(f"tau{tau:g}_S{S}", S, N, K, 4, tau=tau, seed=seed, kcap=True)
      for tau, S, N, K, seed in ((0.5, 40, 3000, 16, 331), (2.0, 40, 3000, 16, 332), (0.5, 64, 3000, 32, 334), (2.0, 64, 3000, 32, 335))),
    *(_small_case(f"rad_pow{p}_C{C}", 40, 3000, 16, 4, C=C, rad_pow=p, seed=340 + i)
      for i, (p, C) in enumerate(((1, 3), (1, 5), (3, 3), (3, 5)))),
)
assert len({c.id for c in CASES}) == len(CASES)


def debug_tol(c):
    """The tolerance tests/test_splat_gpu.py:test_accumulation_modes states for the debug route's features: 1e-6 for alphacomposite and
    wsumnorm at tau = 1, 1e-5 otherwise -- for features of unit magnitude; the compositing is linear in them, so x scale."""
    tight = c.tau == 1.0 and c.acc in ("alphacomposite", "wsumnorm")
    return (1e-6 if tight else 1e-5) * c.scale


def pix_to_ndc(i, S):
    return -1.0 + (2 * i + 1.0) / S


def build(c):
    """(pts (B,N,3), feat (B,C,N)) float32 of a case.  Points are uniform in [-spread, spread]^2 with z in [zlo, zlo + 5]."""
    rs = np.random.RandomState(c.seed)
    pts = np.empty((c.B, c.N, 3), np.float32)
    if c.cloud == "pile":
        # every point within 0.4 px of the centre of output pixel PILE_PIXEL (the caller's x, y: the kernel negates them and tests pixel
        # xi against PixToNdc(S - 1 - xi)), z on a coarse grid: many ties, broken by point index
        px, py = PILE_PIXEL
        jit = (rs.rand(c.B, c.N, 2) * 2 - 1) * 0.4 * (2.0 / c.S)
        pts[..., 0] = pix_to_ndc(px, c.S) + jit[..., 0]
        pts[..., 1] = pix_to_ndc(py, c.S) + jit[..., 1]
        pts[..., 2] = rs.randint(1, c.N // 3, size=(c.B, c.N)).astype(np.float32) * 0.125
    else:
        pts[..., :2] = (rs.rand(c.B, c.N, 2) * 2 - 1) * c.spread
        pts[..., 2] = rs.rand(c.B, c.N) * 5 + c.zlo
        if c.cloud == "corner256":
            # the first workgroup of the last cloud: outside the frame's corner, where the frame clips a footprint to a few tiles
            pts[-1, :BIN_THREADS, :2] = 1.0 + 0.3 * rs.rand(BIN_THREADS, 2)
        for b in range(c.B):                 # holes in a dense cloud (points behind the camera are culled): a mask with islands
            for cx, cy, rad in rs.rand(c.holes, 3) * [1.6, 1.6, 0.15] + [-0.8, -0.8, 0.1]:
                inside = (pts[b, :, 0] - cx) ** 2 + (pts[b, :, 1] - cy) ** 2 < rad ** 2
                pts[b, inside, 2] = -1.0
    feat = ((rs.rand(c.B, c.C, c.N) * 2 - 1) * c.scale).astype(np.float32)
    return pts, feat


def oracle(c, pts, feat):
    """The C oracle on a case (imported here, lazily: this module itself needs nothing built)"""
    from oracle import c_oracle
    return c_oracle.splat_forward(pts, feat, c.S, radius_px=c.r, K=c.K, tau=c.tau, rad_pow=c.rad_pow, accumulation=c.acc,
                                  bg_ksize=c.ksize)


_REF = {}


def reference(c):
    """(pts, feat, oracle result, composite64, E_ref) of a case, computed once per process and shared; treat as read-only"""
    if c.id not in _REF:
        pts, feat = build(c)
        ref = oracle(c, pts, feat)
        c64 = composite64(ref, feat, c.S, c.r, c.rad_pow, c.tau, c.acc)
        for a in (pts, feat, c64, *ref.values()):
            a.setflags(write=False)
        _REF[c.id] = (pts, feat, ref, c64, float(np.abs(ref["feat"] - c64).max()))
    return _REF[c.id]
