"""CPU: the case table of the FID convolution's edge tests (tests/_fid_edge_cases.py) against itself -- every coverage class the GPU
file (tests/test_fid_conv_edges_gpu.py) relies on is present, every case has an output, its integer operands make the convolution
exact in any summation order, and the ReLU leaves at least a quarter of each case's outputs nonzero."""
import numpy as np
import torch

import _fid_edge_cases as E

CASES = E.CASES


def test_limits_and_output_shapes():
    assert len(set(CASES)) == len(CASES)
    for case in CASES + E.SAME_PATCH:
        KH, KW, s, ph, pw, Ci, ldx, Co, N, H, W = case
        assert 1 <= KH <= 7 and 1 <= KW <= 7 and s in (1, 2) and 0 <= ph < KH and 0 <= pw < KW, case
        assert Ci % 4 == 0 and 4 <= Ci <= 20 and ldx in (Ci, Ci + 4, Ci + 12) and 1 <= Co <= 100, case
        assert 1 <= N <= 3 and 1 <= H <= 20 and 1 <= W <= 20, case
        Ho, Wo = E.out_shape(case)
        assert Ho >= 1 and Wo >= 1 and H + 2 * ph >= KH and W + 2 * pw >= KW, case
    assert [E.K_of(c) for c in E.ROUNDING] == [256, 320, 1024, 1040] and all(c[9:] == (9, 9) for c in E.ROUNDING)


def test_output_channel_classes():
    cos = {c[7] for c in CASES}
    assert cos >= {1, 3, 5, 31, 32, 33, 36, 63, 64, 65, 70, 96, 100}
    assert [E.co_tile(co) for co in (1, 32, 33, 64, 65, 96, 97, 100, 128, 129)] == [32, 32, 64, 64, 32, 32, 64, 64, 64, 32]
    blocks = {(E.co_tile(co), -(-co // E.co_tile(co))) for co in cos}
    assert {t for t, _ in blocks} == {32, 64}
    assert {min(n, 3) for _, n in blocks} == {1, 2, 3}, "one, two and three or more Co blocks"
    assert {co % 4 for co in cos} == {0, 1, 2, 3}, "tails of 1, 2 and 3 channels"
    assert any(co % 4 == 0 and co % 16 for co in cos), "a full quad that ends a partial 16-channel tile"
    assert any(co % 16 and co % 4 for co in cos), "a partial 16-channel tile with a scalar tail"
    for T in (32, 64):
        assert any(E.co_tile(co) == T and co > T and co % T for co in cos), f"a partial last Co block at T = {T}"
    assert E.SAME_PATCH[0][7] == 100 and E.SAME_PATCH[1][7] == 70


def test_tap_walk_classes():
    pairs = {(c[0], c[1], c[5]) for c in CASES}
    for kh, kw in E.KERNELS:
        for ci in E.CIS:
            assert (kh, kw, ci) in pairs, (kh, kw, ci)
    Ks = {E.K_of(c) for c in CASES}
    assert {4, 8} <= Ks and max(Ks) <= 980
    assert any(k > 16 and k % 16 for k in Ks) and any(k > 64 and k % 64 for k in Ks)
    S = {E.stages(c) for c in CASES}
    assert {1, 4, 5} <= S and max(S) >= 9, S
    # C4 = 2, 3 and 5 wrap inside a chunk of four groups, under a kernel of more than one tap
    assert {c[5] // 4 for c in CASES if c[0] * c[1] > 1} >= {1, 2, 3, 4, 5}
    assert any(c[0] % 2 == 0 and c[1] % 2 == 0 for c in CASES) and any((c[0], c[1], c[2]) == (5, 5, 2) for c in CASES)


def test_stride_and_padding_classes():
    for pad in ((1, 1), (2, 2), (3, 3), (0, 2), (2, 0)):
        hit = [c for c in CASES if c[2] == 2 and (c[3], c[4]) == pad]
        assert {c[9] % 2 for c in hit} == {0, 1} and {c[10] % 2 for c in hit} == {0, 1}, (pad, hit)
    assert any(c[2] == 2 and (c[3], c[4]) == (0, 2) and c[0] == c[1] for c in CASES), "asymmetric padding on a square kernel"
    assert any(c[2] == 1 and c[3] == c[0] - 1 >= 1 and c[4] == c[1] - 1 >= 1 for c in CASES), "stride 1 with padding KH - 1, KW - 1"
    for k in range(1, 7):
        assert any(c[2] == 1 and (c[3] == k or c[4] == k) for c in CASES), f"stride 1 with a padding of {k}"


def test_small_map_classes():
    assert any(c[:5] == (3, 3, 1, 1, 1) and c[9:] == (1, 1) for c in CASES)
    assert any(c[:5] == (1, 7, 1, 0, 3) and c[10] == 2 for c in CASES)
    assert any(c[9] + 2 * c[3] == c[0] and c[3] > 0 for c in CASES), "H + 2 ph == KH"
    assert any(c[:5] == (7, 7, 1, 3, 3) and c[9:] == (4, 4) for c in CASES)
    assert any(c[10] < c[1] for c in CASES) and any(c[9] < c[0] for c in CASES), "a map narrower / lower than the kernel"


def test_pixel_count_classes():
    counts = {E.pixels(c) for c in CASES}
    assert {1, 15, 16, 17, 128} <= counts
    by_tile = {T: {E.pixels(c) for c in CASES if E.co_tile(c[7]) == T} for T in (32, 64)}
    # no N <= 3, Ho, Wo <= 20 multiply to 127 (a prime): 126 is the count just under the 128-pixel tile
    assert {126, 128} <= by_tile[64] and any(128 < n <= 132 for n in by_tile[64]) and any(n > 256 for n in by_tile[64])
    assert {255, 256} <= by_tile[32] and any(256 < n <= 260 for n in by_tile[32])
    assert any(n > 128 and n % 128 for n in by_tile[64]) and any(n > 256 and n % 256 for n in by_tile[32]), "a ragged last tile of several"
    for case in E.SAME_PATCH:
        per = 128 if E.co_tile(case[7]) == 64 else 256
        assert E.pixels(case) > per and E.pixels(case) % per, case


def test_input_width_classes():
    assert {c[6] - c[5] for c in CASES} == {0, 4, 12}
    for T in (32, 64):
        assert {c[6] - c[5] for c in CASES if E.co_tile(c[7]) == T} == {0, 4, 12}


def test_integer_operands_are_exact_and_leave_a_quarter_nonzero():
    least = 1.0
    for k, case in enumerate(CASES):
        x, w, b = E.integer_operands(k)
        K = E.K_of(case)
        for a, lim in ((x, 3), (w, 3), (b, 8)):
            assert a.dtype == np.float32 and np.array_equal(a, np.round(a)) and float(np.abs(a).max()) <= lim
        assert K <= 980 and 9 * K + 8 < 2 ** 24
        want = E.reference(x, w, b, case)
        assert tuple(want.shape) == (case[8],) + E.out_shape(case) + (case[7],)
        assert bool((want == want.round()).all()) and float(want.max()) <= 9 * K + 8
        assert torch.equal(want.float().double(), want), "the reference is exact in float32"
        frac = float((want > 0).double().mean())
        least = min(least, frac)
        assert frac >= 0.25, (E.name(case), frac)
        # the widened map holds NaN behind the channels the layer reads and nowhere else
        wide = E.widen(x, case[6])
        assert np.array_equal(wide[..., :case[5]], x) and np.isnan(wide[..., case[5]:]).all()
    print(f"{len(CASES)} cases, smallest nonzero fraction {least:.3f}")


def test_same_patch_operands_give_one_positive_value():
    for k, case in enumerate(E.SAME_PATCH):
        x, w, b, value = E.same_patch_operands(case, 300 + k)
        want = E.reference(x, w, b, case)
        assert value > 0 and float((want - value).abs().max()) <= 1e-12 * max(1.0, value), (case, value)
        assert bool((w == w[:1]).all()) and bool((b == b[0]).all())
