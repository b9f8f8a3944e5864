"""The cases of tests/_splat_ref.py, checked without a GPU: every case reaches the branch of pixelsynth_amd/csrc/splat_pipeline.h it is there for
(asserted with the numpy mirror of the binning, _splat_ref.bins), and its reference is usable -- the oracle's fp32 features lie within
2e-6 x max |feature| of the float64 compositing of the oracle's own hit lists (5e-8 ... 1.0e-6 here, the largest at tau = 0.5), the mask
has hit and missed pixels where the case looks at it, and pixels with K hits exist where the case is about the K cap.
tests/test_splat_routes_gpu.py runs the same table on the device."""
import numpy as np
import pytest

import _splat_ref as R


def _small(c, b, ref):
    """One of the small frames of the composite cases: every list in one wave's reach, the LDS routes of the binning"""
    assert b.NT <= R.SCAN_THREADS and b.counts.max() <= R.SORT_SMALL_CAP and b.foot.max() <= R.MAX_TPP
    assert (b.foot == 0).any() and c.route == "both"          # (some points are culled)


def fill_mixed(c, b, ref):
    """k_bin_fill: at least one workgroup of 256 consecutive points holds a live footprint > 9 tiles (the direct path) and at least one
    holds none (the LDS path), so the workgroup-uniform decision goes both ways in one launch; lists for k_sort_big; true division"""
    direct = R.fill_workgroups(b)
    assert b.NT <= R.LDS_TILES and direct.any() and not direct.all()
    assert not direct[-1, 0] and (b.foot[-1, :R.BIN_THREADS] > 0).any()      # (the corner workgroup is live, and fits)
    assert (b.foot > R.MAX_TPP).sum() > c.N // 4 and b.foot.max() <= b.max_tiles_pp
    assert (b.counts > R.SORT_SMALL_CAP).any()
    assert not R.recip_route(c.S, c.r, c.rad_pow)


def whole_frame(c, b, ref):
    """The largest radius the entry point accepts: a footprint is the whole frame, far more than MAX_TPP"""
    assert c.r == 64 and b.foot.max() == b.NT and b.max_tiles_pp == 324 and b.foot.max() <= b.max_tiles_pp


def scan_per(c, b, ref):
    """k_scan: `arg` counters per thread, threads whose first counter lies past NT, and lists behind the first 1024 tiles"""
    per = (b.NT + R.SCAN_THREADS - 1) // R.SCAN_THREADS
    assert per == c.arg and (R.SCAN_THREADS - 1) * per >= b.NT and b.NT <= R.LDS_TILES
    assert (b.counts[:, R.SCAN_THREADS:] > 0).all() and (b.counts[:, -b.tilesX:] > 0).all()
    if c.S % R.TILE:
        assert b.tilesX == (c.S + R.TILE) // R.TILE                          # (a partial last tile)


def nt_gt_lds(c, b, ref):
    """More tiles than LDS counters: k_bin_count and k_bin_fill go straight to the global counters"""
    assert b.NT > R.LDS_TILES and R.fill_workgroups(b).all()
    assert (b.counts[:, R.LDS_TILES:] > 0).any()
    assert (c.S % 64 == 0) == c.id.endswith("bits") and c.S // 64 <= R.DB_MAXW


def tile_255(c, b, ref):
    """The size limit: tile coordinate 255 in the 8-bit bbox packing, DB_MAXW words per row of the mask"""
    assert c.S == 2048 and b.tilesX - 1 == 255 and c.S // 64 == R.DB_MAXW
    cnt = b.counts.reshape(c.B, b.tilesX, b.tilesX)
    assert cnt[:, 255, :].any() and cnt[:, :, 255].any() and cnt[:, 0, :].any() and cnt[:, :, 0].any()
    hit = ref["idx"][..., 0] >= 0                                              # hit pixels in all four border tile rows and columns
    assert hit[:, -R.TILE:, :].any() and hit[:, :, -R.TILE:].any() and hit[:, :R.TILE, :].any() and hit[:, :, :R.TILE].any()


def one_list(c, b, ref):
    """Exactly one non-empty list, of exactly n keys: the size switch of the sorts at and one past every cap; some pixels see the whole
    list, so their idx rows ARE the sorted list"""
    assert (b.counts > 0).sum() == 1 and b.counts.max() == c.arg == c.N == c.K
    px, py = R.PILE_PIXEL
    assert np.flatnonzero(b.counts[0])[0] == (py // R.TILE) * b.tilesX + px // R.TILE
    full = ref["idx"][..., c.K - 1] >= 0
    assert full.sum() >= 5 and full[0, py, px]
    z = ref["zbuf"][0, py, px]
    assert (np.diff(z) == 0).sum() > c.N // 2                                  # (z ties, broken by index)


def big_lists(c, b, ref):
    """More lists queued for k_sort_big than it has workgroups: the second trip of its grid-stride loop"""
    queued = (b.counts > R.SORT_SMALL_CAP).sum()
    assert queued > c.arg == R.SORT_BIG_WGS and b.counts.max() <= R.SORT_BIG_CAP


def division(c, b, ref):
    """A radius for which (2 r / S)^rad_pow is no power of two: RECIP = false"""
    _small(c, b, ref)
    assert not R.recip_route(c.S, c.r, c.rad_pow)


def partial_recip(c, b, ref):
    """A size that is no multiple of the tile (lanes past the frame) at a power-of-two denominator: RECIP = true"""
    _small(c, b, ref)
    assert c.S % R.TILE and R.recip_route(c.S, c.r, c.rad_pow)


def small(c, b, ref):
    _small(c, b, ref)
    if c.C != 3:
        assert (c.C % 4 != 0) == (c.C in (5, 7)) and c.acc == "alphacomposite"


BRANCHES = dict(fill_mixed=fill_mixed, whole_frame=whole_frame, scan_per=scan_per, nt_gt_lds=nt_gt_lds, tile_255=tile_255,
                one_list=one_list, big_lists=big_lists, division=division, partial_recip=partial_recip, small=small)


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_case_reaches_its_branch_and_its_reference_is_usable(c):
    pts, feat, ref, c64, e_ref = R.reference(c)
    b = R.bins(pts, c.S, c.r)
    BRANCHES[c.branch](c, b, ref)
    # the mirror against the oracle: a pixel with a hit lies in a tile with a non-empty list
    hit = ref["idx"][..., 0] >= 0
    ty, tx = np.arange(c.S) // R.TILE, np.arange(c.S) // R.TILE
    assert not (hit & (b.counts.reshape(c.B, b.tilesX, b.tilesX)[:, ty][:, :, tx] == 0)).any()
    fmax = float(np.abs(feat).max())
    print(f"{c.id}: E_ref = {e_ref:.3g} (x max |feature| {fmax:.3g}: {e_ref / fmax:.3g}), bg.mean = {ref['bg'].mean():.4f}, "
          f"pixels with K hits = {(ref['idx'][..., c.K - 1] >= 0).mean():.4f}, NT = {b.NT}, longest list = {b.counts.max()}, "
          f"largest footprint = {b.foot.max()}")
    assert e_ref <= R.ORACLE_VS_F64 * fmax
    assert np.abs(c64).max() > 0.1 * fmax
    if c.mask == "mean":
        assert 0.005 < ref["bg"].mean() < 0.995
    elif c.mask == "both":
        assert ref["bg"].any() and not ref["bg"].all() and hit.any() and not hit.all()
    if c.kcap:
        assert (ref["idx"][..., c.K - 1] >= 0).any()


def test_sort_cases_stand_at_and_one_past_every_cap():
    """64 / 128 / 256 keys: the keys per lane of the register sort; 512: k_sort_small -> k_sort_big; 1024: one key per thread of
    k_sort_big; 8192: its LDS -> global memory"""
    for cap in (*R.SORT_REG_CAPS, R.SCAN_THREADS, R.SORT_BIG_CAP):
        assert cap in R.SORT_LENGTHS and cap + 1 in R.SORT_LENGTHS
    assert {c.arg for c in R.CASES if c.branch == "one_list"} == set(R.SORT_LENGTHS)


def test_composite64_is_the_oracle_at_a_golden_configuration():
    """composite64 against the oracle where the suite already trusts it (tau = 1, rad_pow = 2, alphacomposite, S = 32), and its three
    accumulations against a direct loop over one pixel"""
    c = R._case("plain", 32, 700, 8, 4, seed=1, spread=1.2, zlo=-0.2)
    pts, feat = R.build(c)
    ref = R.oracle(c, pts, feat)
    assert np.abs(R.composite64(ref, feat, 32, 4, 2, 1.0, "alphacomposite") - ref["feat"]).max() < 1e-6
    y, x = np.argwhere(ref["idx"][0, :, :, 3] >= 0)[0]
    n, d = ref["idx"][0, y, x], ref["dist"][0, y, x].astype(np.float64)
    k = n >= 0
    a = (1 - np.sqrt(np.clip(d[k] / float(np.float32((2 * 4 / 32) ** 3)), float(np.float32(1e-3)), 1))) ** 0.5
    f = feat[0, 1, n[k]].astype(np.float64)
    acc, cum = 0.0, 1.0
    for ai, fi in zip(a, f):
        acc, cum = acc + cum * ai * fi, cum * (1 - ai)
    want = dict(alphacomposite=acc, wsum=(a * f).sum(), wsumnorm=(a * f).sum() / max(a.sum(), float(np.float32(1e-4))))
    for mode, w in want.items():
        got = R.composite64(ref, feat, 32, 4, 3, 0.5, mode)[0, 1, y, x]
        assert abs(got - w) < 1e-12, mode


def test_bins_matches_a_direct_count():
    """bins() against a per-point loop over tiles, culled points (z < 0, NaN, inf, far outside) included"""
    c = R._case("direct", 44, 500, 4, 5, seed=3, spread=1.3, zlo=-0.5)
    pts, _ = R.build(c)
    pts[0, :3, 0] = np.inf
    pts[0, 3:6, 1] = np.nan
    pts[1, :3, 2] = np.nan
    b = R.bins(pts, c.S, c.r)
    assert b.tilesX == 6 and b.NT == 36 and (b.foot[0, :6] == 0).all() and (b.foot[1, :3] == 0).all()
    f = np.float32
    for bi in range(2):
        cnt = np.zeros(36, int)
        for n in range(c.N):
            if not pts[bi, n, 2] >= 0:
                continue
            rng = []
            for p in (-pts[bi, n, 0], -pts[bi, n, 1]):
                cc = f(f(f(f(p + f(1)) * f(44)) - f(1)) * f(0.5))
                lo, hi = f(cc - b.hw), f(cc + b.hw)
                if not hi >= 0 or not lo <= 43:
                    break
                ilo, ihi = int(np.ceil(max(lo, f(0)))), int(np.floor(min(hi, f(43))))
                if ilo > ihi:
                    break
                rng.append(((43 - ihi) // 8, (43 - ilo) // 8))
            if len(rng) == 2:
                for ty in range(rng[1][0], rng[1][1] + 1):
                    for tx in range(rng[0][0], rng[0][1] + 1):
                        cnt[ty * 6 + tx] += 1
                assert b.foot[bi, n] == (rng[0][1] - rng[0][0] + 1) * (rng[1][1] - rng[1][0] + 1)
            else:
                assert b.foot[bi, n] == 0
        assert np.array_equal(cnt, b.counts[bi])
