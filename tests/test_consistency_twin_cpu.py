"""CPU: the float32 twin of the consistency kernel (tests/_consistency_twin.py) before it judges the kernel
(tests/test_consistency_shapes_gpu.py): against the fp64 restatement, its block walk against the vectorised rule, the conditions the
case table must meet for the GPU test to mean something, and that the twin tells the slips it is there to catch."""
import os
import re

import numpy as np
import pytest

import _consistency_twin as T
import consistency_ref64 as R
import percsim_ref64 as PR
from test_consistency_gpu import BOUND_PSNR, BOUND_WARP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ["%dx%d" % s for s in T.SHAPES]


def _scale255(ta):
    """RAW mode's t * 2 - 1 back on the 0-255 scale, in fp64"""
    return (ta.astype(np.float64) + 1.0) / 2.0 * 255.0


def test_twin_against_the_fp64_restatement():
    # From the operations: 255 * 2^-24 for the four products plus 3 * 0.5 ulp(255) for the three additions, about 3.8e-5 on the 0-255
    # scale; the readback below (/ 255, * 2 - 1 in fp32, then back in fp64) adds what tests/test_consistency_gpu.py's own adds.
    worst, worst_psnr = 0.0, 0.0
    for H, W in T.SHAPES:
        ones = np.ones((T.B, 1, H, W), np.float32)
        for family in ("mild", "outside"):
            maps = T.family_maps(H, W, family)
            for dtype in (np.uint8, np.float32):
                v1, v2 = T.views(H, W, dtype)
                ta, _, _ = T.twin_batch(v1, v2, ones, ones, maps)
                for i in range(T.B):
                    for k, (src, _, _) in enumerate(T.directions(v1, v2, ones, ones)):
                        want = R.warp64(R.try_bgr(src[i]), maps[i, k])
                        worst = max(worst, float(np.abs(_scale255(ta[i, k]) - want).max()))
                for kind in T.MASK_KINDS:
                    m1, m2 = T.masks(H, W, kind)
                    _, _, sums = T.twin_batch(v1, v2, m1, m2, maps)
                    for i in range(T.B):
                        for k, (src, ref, m) in enumerate(T.directions(v1, v2, m1, m2)):
                            want = R.direction64(src[i], ref[i], m[i], maps[i, k])[0]
                            worst_psnr = max(worst_psnr, abs(float(T.psnr_of(*sums[i, k])) - want))
    print("twin max error against fp64 (0-255 scale): %.3g;  PSNR against direction64 (dB): %.3g" % (worst, worst_psnr))
    assert worst <= BOUND_WARP
    assert worst_psnr <= BOUND_PSNR


@pytest.mark.parametrize("H,W", T.SHAPES, ids=IDS)
def test_block_walk_equals_the_vectorised_rule(H, W):
    for family in T.FAMILIES:
        for i, pair in enumerate(T.family_maps(H, W, family)):
            for k, M in enumerate(pair):
                got, want = T.source_positions_loop(M, H, W), T.positions_of(M, H, W)
                for g, w_, name in zip(got, want, ("sx", "sy", "fx", "fy")):
                    assert np.array_equal(g, w_), (family, i, k, name)


def _in_view(M, H, W):
    """-> (taps inside (4, H, W), taps inside with a nonzero weight (4, H, W), fx, fy)"""
    sx, sy, fx, fy = T.positions_of(M, H, W)
    ok = T.taps_inside(sx, sy, H, W)
    return ok, ok & (np.stack(T.weights(fx, fy)) != 0), fx, fy


@pytest.mark.parametrize("H,W", T.SHAPES, ids=IDS)
def test_case_table_reaches_what_it_is_there_for(H, W):
    counts, frac = [], {}
    for family in ("mild", "outside"):
        for i, pair in enumerate(T.family_maps(H, W, family)):
            for k, M in enumerate(pair):
                ok, seen, fx, fy = _in_view(M, H, W)
                assert seen.any(0).mean() >= 0.5, (family, i, k, "pixels with a weighted tap in view: %.2f" % seen.any(0).mean())
                frac[family] = frac.get(family, False) or bool((fx | fy).any())
                counts.append(ok.sum(0))
    counts = np.stack(counts)
    assert frac == {"mild": True, "outside": True}, "a nonzero fraction in every case"
    if H >= 2 and W >= 2:
        assert (counts == 4).any() and ((counts > 0) & (counts < 4)).any() and (counts == 0).any()
    else:
        assert (counts > 0).any() and (counts < 4).all()          # a single row or column: a neighbour tap is always outside
    # the saturating family: each map does what its name says, at some pixel of this shape
    maps = T.family_maps(H, W, "saturating").reshape(-1, 9)
    assert len(maps) == len(T.SATURATING)
    assert any((fx | fy).any() for _, _, fx, fy in (_in_view(M, H, W) for M in maps))
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for kind, M in zip(T.SATURATING, maps):
        with np.errstate(all="ignore"):
            w = M[6] * xx + M[7] * yy + M[8]
            px, py = (M[0] * xx + M[1] * yy + M[2]) / w, (M[3] * xx + M[4] * yy + M[5]) / w
        if kind == "scale400":
            low = (np.floor(px) < -32768) | (np.floor(py) < -32768)
            high = (np.floor(px) > 32767) | (np.floor(py) > 32767)
            assert low.any() and (high.any() or H * W == 1) and max(np.abs(32 * px).max(), np.abs(32 * py).max()) < 2.0 ** 31
        elif kind == "scale1e9":
            assert ((np.abs(32 * px) > 2.0 ** 31) | (np.abs(32 * py) > 2.0 ** 31)).any()
            if H > 1 and W > 1:
                assert _in_view(M, H, W)[1][0, H // 2, W // 2], "the centre pixel reads the source's (0, 0)"
        elif kind == "w_crosses_0":
            assert (w == 0).any()
            sx, sy, fx, fy = T.positions_of(M, H, W)
            assert all((a[w == 0] == 0).all() for a in (sx, sy, fx, fy))
        elif kind == "nan":
            assert np.isnan(M).any()
        else:
            assert np.isinf(M).any()
    sx, sy, fx, fy = T.positions_of(maps[T.SATURATING.index("inf_w")], H, W)
    assert not sx.any() and not sy.any() and not fx.any() and not fy.any()      # 32 / inf = 0: everything reads (0, 0)


def test_block_edges_fall_inside_tiles():
    assert [T.block_of(*s) for s in T.SHAPES] == [(1, 1), (1, 1024), (3, 7), (5, 204), (12, 85), (15, 68), (16, 64), (16, 64), (16, 37)]
    for H, W in ((5, 300), (12, 200), (15, 70)):
        bw0 = T.block_of(H, W)[1]
        assert any(e % T.TX for e in range(bw0, W, bw0)), (H, W)
    # the tile counts the GPU test's launches have: 18 at 1 x 1100, one partial tile at 3 x 7, a one-column second tile at 17 x 65
    tiles = lambda H, W: (-(-W // T.TX), -(-H // T.TY))
    assert tiles(1, 1100) == (18, 1) and tiles(3, 7) == (1, 1) and tiles(17, 65) == (2, 5) and tiles(6, 70) == (2, 2)
    assert 15 % 4 == 3 and 17 % 4 == 1


def test_transposed_pair_holds_the_same_data():
    for dtype in (np.uint8, np.float32):
        for a, b in zip(T.views(37, 130, dtype), T.views(130, 37, dtype)):
            assert np.array_equal(a.transpose(0, 1, 3, 2), b)
    for kind in T.MASK_KINDS:
        for a, b in zip(T.masks(37, 130, kind), T.masks(130, 37, kind)):
            assert np.array_equal(a.transpose(0, 1, 3, 2), b)
    # and the maps send the transposed pixel to the transposed position (the block rule aside: an exact map shows it)
    M = T.family_maps(37, 130, "mild")[1, 0].reshape(3, 3)
    Mt = T.family_maps(130, 37, "mild")[1, 0].reshape(3, 3)
    p = np.array([5.0, 9.0, 1.0])
    q, qt = M @ p, Mt @ p[[1, 0, 2]]
    assert np.allclose(q[:2] / q[2], (qt[:2] / qt[2])[::-1], rtol=1e-12, atol=0)


def test_twin_tells_a_tile_origin_from_the_block_origin():
    # the slip: xb = (x / 64) * 64, the tile's first column, in place of the block's.  On a square of 256 the two coincide; at 5 x 300
    # (bw0 = 204) every column from 64 on is counted from another origin, and on the tie map fp64's last bits then fall the other way
    H, W = 5, 300
    M = T.family_maps(H, W, "mild")[0, 0]
    assert np.array_equal(M.reshape(3, 3), T.tie_map())
    right, slip = T.source_positions_loop(M, H, W), T.source_positions_loop(M, H, W, bw0=T.TX)
    moved = (right[2] != slip[2]) | (right[0] != slip[0])
    assert moved.any() and not moved[:, :T.TX].any(), "the first tile starts where the first block does"
    v1, v2 = T.views(H, W, np.uint8)
    m1, _ = T.masks(H, W, "f32")
    ta = T.twin32(v2[0], v1[0], m1[0], M)[0]
    tb = T.twin32(v2[0], v1[0], m1[0], M, positions=slip)[0]
    worst = float(np.abs(_scale255(ta) - _scale255(tb)).max())
    print("tile-origin slip: %d pixels move, the warp by up to %.3g on the 0-255 scale" % (moved.sum(), worst))
    assert worst > 1e4 * BOUND_WARP


def test_twin_tells_a_mask_indexed_with_h_and_w_swapped():
    # the slip: (item * W + y) * H + x.  Invisible on a square; at 37 x 130 it reads another pixel's mask (and stays inside the buffer)
    H, W = 37, 130
    M = T.family_maps(H, W, "mild")[1, 1]
    v1, v2 = T.views(H, W, np.float32)
    _, m2 = T.masks(H, W, "f32")
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    assert (yy * H + xx).max() < H * W
    swapped = m2[1].ravel()[yy * H + xx][None]
    ta = T.twin32(v1[1], v2[1], m2[1], M)
    tb = T.twin32(v1[1], v2[1], swapped, M)
    worst = float(np.abs(_scale255(ta[0]) - _scale255(tb[0])).max())
    assert worst > 1e4 * BOUND_WARP


def test_pnet_constants_cannot_drift():
    from pixelsynth_amd.networks import pretrained_networks as PN
    assert np.array_equal(T.PNET_SHIFT, PR.SHIFT) and np.array_equal(T.PNET_SCALE, PR.SCALE)
    assert T.PNET_SHIFT.dtype == np.float32 and T.PNET_SCALE.dtype == np.float32
    net = PN.PNet(pnet_rand=True, use_gpu=False)
    assert np.array_equal(net.shift.numpy().ravel(), T.PNET_SHIFT) and np.array_equal(net.scale.numpy().ravel(), T.PNET_SCALE)
    text = open(os.path.join(ROOT, "pixelsynth_amd", "csrc", "ps_image.h")).read()
    for name, want in (("c_pnet_shift", T.PNET_SHIFT), ("c_pnet_scale", T.PNET_SCALE)):
        body = re.search(name + r"\[3\] = \{([^}]*)\}", text).group(1)
        assert np.array_equal(np.array([np.float32(v.strip().rstrip("f")) for v in body.split(",")]), want), name
    t = np.array([-1.0, 0.25, 1.0], np.float32)
    for j in range(3):
        want = ((t.astype(np.float64) - float(T.PNET_SHIFT[j])).astype(np.float32).astype(np.float64) / float(T.PNET_SCALE[j]))
        assert np.array_equal(T.standardised(t, j), want.astype(np.float32))


def test_psnr_formula_and_its_helpers():
    assert T.psnr_of(0.0, 5.0) == 100.0 and T.psnr_of(0.0, 0.0) == 100.0 and T.psnr_of(1e-12, 4.0) == 100.0
    assert np.isnan(T.psnr_of(np.nan, 2.0)) and np.isnan(T.psnr_of(np.nan, np.nan))
    assert T.psnr_of(3.0, 0.5) == np.float32(0.0) and T.psnr_of(3.0, 10.0) == np.float32(10.0)     # the clamp of the mask sum at 1
    assert T.psnr_of(np.inf, 2.0) == -np.inf
    assert T.psnr_of(0.75, 2.5) == np.float32(10.0 * np.log10(3.0 * 2.5 / 0.75))
    one = np.float32(1.0)
    assert T.ulp_distance(one, np.nextafter(one, np.float32(2))) == 1 and T.ulp_distance(np.nan, np.nan) == 0
    assert T.ulp_distance(one, np.nan) == 2 ** 31 and T.ulp_distance(one, -one) == 2 ** 31
    mid = 0.5 * (1.0 + float(np.nextafter(one, np.float32(2))))
    assert not T.rounding_is_safe(mid) and not T.rounding_is_safe(mid * (1 + 1e-12)) and T.rounding_is_safe(1.0)
    assert T.rounding_is_safe(float("nan"))


def test_twin_hands_non_finite_values_on():
    H, W = 3, 7
    v1, v2 = (v.copy() for v in T.views(H, W, np.float32))
    m1, _ = T.masks(H, W, "f32")
    ident = np.eye(3).ravel()
    v2[0, 1, 1, 2] = np.nan                    # the source: RGB channel 1 = BGR channel 1
    v2[0, 0, 2, 6] = np.inf                    # BGR channel 2
    ta, tb, sd, sm = T.twin32(v2[0], v1[0], m1[0], ident)
    # under the identity the weights are (1, 0, 0, 0): the NaN pixel itself, and its left and upper neighbours through NaN * 0
    nan_at = {(1, 2), (1, 1), (0, 2), (0, 1)}
    assert {(y, x) for y, x in zip(*np.nonzero(np.isnan(ta[..., 1])))} == nan_at
    # inf * 1 = inf at the pixel, inf * 0 = NaN left of and above it; the frame's edge has no tap to the right of it
    assert np.isinf(ta[2, 6, 2]) and np.isnan(ta[2, 5, 2]) and np.isnan(ta[1, 6, 2]) and np.isnan(ta[1, 5, 2])
    assert np.isfinite(tb).all() and np.isnan(sd) and np.isfinite(sm) and np.isnan(T.psnr_of(sd, sm))
