"""The route cases of tests/_splat_bwd_ref.py, tests/_vq_train_ref.py and tests/_lmconv_bwd_ref.py, checked without a GPU: every case
reaches the branch of csrc/splat_bwd.hip, csrc/vq_train.hip or csrc/lmconv_bwd.hip it is there for -- asserted on the trip counts of the
splat's two channel loops and on the Python mirrors of the other two kernels' plans, whose workspace sizes are held to the libraries' own
-- and no shape of the operator tests reaches it already, so a case that adds nothing is caught.  tests/test_train_routes2_gpu.py runs
the same tables on the device."""
import pytest

import _lmconv_bwd_ref as L
import _splat_bwd_ref as S
import _splat_ref as sr
import _vq_train_ref as V
from pixelsynth_amd import _lib


# ---- the splat's backward pass ---------------------------------------------------------------------------------------------------------------
OPERATOR_CASES = [c for c in sr.CASES if c.id in S.OPERATOR_CASE_IDS]
SPLAT_FIGURES = {       # case -> (C, pixel_chunks, C % 8, box_walks, lanes that own a channel in the last walk)
    "bwd_C13_wsumnorm": (13, 2, 5, 1, 13),
    "bwd_C16": (16, 2, 0, 1, 16),
    "bwd_C64": (64, 8, 0, 1, 64),
    "bwd_C70_tau2": (70, 9, 6, 2, 6),
    "bwd_C130_wsum": (130, 17, 2, 3, 2),
    "bwd_K1": (9, 2, 1, 1, 9),
}


def test_no_operator_case_of_the_splat_takes_a_second_chunk():
    assert len(OPERATOR_CASES) == len(S.OPERATOR_CASE_IDS) and {c.C for c in OPERATOR_CASES} == {3, 5, 8}
    assert all(S.pixel_chunks(c.C) == 1 and S.box_walks(c.C) == 1 and c.K > 1 for c in OPERATOR_CASES)
    assert not {c.id for c in S.ROUTE_CASES} & {c.id for c in sr.CASES} and len({c.id for c in S.ROUTE_CASES}) == len(S.ROUTE_CASES)
    assert [S.pixel_chunks(C) for C in (1, 8, 9, 16, 17)] == [1, 1, 2, 2, 3] and [S.box_walks(C) for C in (1, 64, 65, 128, 129)] == [1, 1, 2, 2, 3]
    assert {c.acc for c in S.ROUTE_CASES} == {"alphacomposite", "wsum", "wsumnorm"} and sum(c.N == 300 for c in S.ROUTE_CASES) == 2


@pytest.mark.parametrize("case", S.ROUTE_CASES, ids=lambda c: c.id)
def test_splat_case_reaches_its_branch(case):
    c = case
    walks = S.box_walks(c.C)
    assert (c.C, S.pixel_chunks(c.C), c.C % S.QCH, walks, c.C - (walks - 1) * S.LANES) == SPLAT_FIGURES[c.id]
    assert S.pixel_chunks(c.C) > 1 and c.tau >= 1.0 and (c.K == 1) == (c.id == "bwd_K1")
    pts, feat, o, _, _ = sr.reference(c)
    idx = o["idx"]
    seen, kink = S.hit_points(idx, c.B, c.N), S.kink_points(c, idx, o["dist"], c.B, c.N)
    full = float((idx[..., -1] >= 0).mean())
    print(f"{c.id}: {seen.sum()} of {c.B * c.N} points seen, {kink.sum()} near a clamp bound, {full:.0%} of the lists full, "
          f"{float((idx[..., 0] < 0).mean()):.0%} empty")
    assert seen.any() and (~seen).any() and kink.sum() <= 0.02 * seen.sum()
    if c.K == 8:                                                              # (at K = 1 and K = 4 every list of these clouds is full)
        short = ((idx[..., 0] >= 0) & (idx[..., -1] < 0)).mean()
        assert short > (0.25 if c.N == 300 else 0.0)                          # lists that end in -1 before K: a good share at N = 300
    # the largest tensor of the host reference: the formula's (B, C, S, S, K) gather
    assert c.B * c.C * c.S * c.S * c.K < 1e6


# ---- the training quantiser ------------------------------------------------------------------------------------------------------------------
VQ_REACHES = {       # case -> the property no operator shape has, on (the plan, D, K)
    "dt3_parts3": lambda p, D, K: p.dt == 3 and D % V.TILE == 1 and p.kt % 2 == 1 and p.kt > 1 and p.parts > 1 and p.qwgs > 1 and V.Q_ELEMS % D != 0,
    "dt3_one_code_tile": lambda p, D, K: p.dt == 3 and D % V.TILE == 0 and p.kt == 1 and p.wpp == 1 and p.parts > 1,
    "dt2": lambda p, D, K: p.dt == 2 and p.wpp > 1 and p.parts > 1,
    "dt2_edge": lambda p, D, K: p.dt == 2 and D % V.TILE == 1 and p.qwgs > 1 and V.Q_ELEMS % D != 0,
    "dt1_quantize_walk": lambda p, D, K: p.dt == 1 and p.parts > 1 and p.qwgs > 1 and V.Q_ELEMS % D != 0,
}
VQ_FIGURES = {       # case -> (dt, kt, wpp, part_rows, parts, qwgs, 16384 % D: the channel k_quantize's second workgroup starts at)
    "dt3_parts3": (3, 3, 2, 512, 3, 3, 16),
    "dt3_one_code_tile": (3, 1, 1, 512, 2, 3, 16),
    "dt2": (2, 7, 4, 512, 2, 1, 4),
    "dt2_edge": (2, 3, 2, 512, 3, 2, 13),
    "dt1_quantize_walk": (1, 3, 2, 512, 7, 2, 4),
}


@pytest.mark.parametrize("case", V.ROUTE_CASES, ids=lambda c: c.id)
def test_vq_case_reaches_its_branch(case):
    N, D, K = case.shape
    p = V.plan(N, D, K)
    print(case.id, p)
    ws = _lib.library("vq_train").ps_vq_train_workspace_bytes
    assert p.bytes == ws(N, D, K) and tuple(p[:6]) + (V.Q_ELEMS % D,) == VQ_FIGURES[case.id]
    assert VQ_REACHES[case.id](p, D, K), case.why
    for old in V.OPERATOR_SHAPES:
        q = V.plan(*old)
        assert q.bytes == ws(*old)
        assert not VQ_REACHES[case.id](q, old[1], old[2]), (case.id, old)
        # what the operator shapes leave out altogether: DT = 2 and 3, one code tile, parts at DT < 4, a workgroup of k_quantize off channel 0
        assert q.dt in (1, 4) and q.kt > 1 and (q.parts == 1 or q.dt == 4) and (q.qwgs == 1 or V.Q_ELEMS % old[1] == 0), old
    assert N * D <= 1e5


def test_the_vq_cases_cover_the_dispatch():
    assert {V.plan(*c.shape).dt for c in V.ROUTE_CASES} == {1, 2, 3} and len({c.id for c in V.ROUTE_CASES}) == 5
    assert V.plan(1, 1, 1)[:6] == (1, 1, 1, 512, 1, 1) and V.plan(65537, 64, 512)[:6] == (4, 32, 16, 1024, 65, 257)


# ---- the locally masked convolution's backward pass -------------------------------------------------------------------------------------------
LM_REACHES = {       # case -> the property no operator shape has, on (the plan, the shape)
    "chunk6_short_last": lambda p, s: p.chunk % L.DEPTH != 0 and p.chunk > 2 and p.last < p.chunk,
    "chunk6_d2": lambda p, s: p.chunk % L.DEPTH != 0 and p.chunk > 2 and s[5] > 1,
    "chunk3": lambda p, s: p.chunk % L.DEPTH != 0 and p.chunk > 2 and p.last < p.chunk and p.chunk < L.DEPTH,
    "grid_1x1": lambda p, s: s[3] * s[4] < L.KSTEP and p.N < 8,
    "grid_2x1_d2": lambda p, s: s[4] == 1 and s[5] >= max(s[3], s[4]) and p.N < 8,
    "grid_3x3": lambda p, s: s[4] < L.KSTEP and s[3] > 1,
    "row_1x3": lambda p, s: s[3] == 1 and s[4] > 1,
    "dilation_past_grid": lambda p, s: s[5] >= min(s[3], s[4]) and s[3] * s[4] > 9,
}
LM_FIGURES = {       # case -> (N, ksteps, chunk, parts, last)
    "chunk6_short_last": (1290, 323, 6, 54, 5),
    "chunk6_d2": (1295, 324, 6, 54, 6),
    "chunk3": (256, 64, 3, 22, 1),
    "grid_1x1": (5, 2, 1, 2, 1),
    "grid_2x1_d2": (6, 2, 1, 2, 1),
    "grid_3x3": (18, 5, 1, 5, 1),
    "row_1x3": (21, 6, 1, 6, 1),
    "dilation_past_grid": (108, 27, 1, 27, 1),
}


@pytest.mark.parametrize("case", L.ROUTE_CASES, ids=lambda c: c.id)
def test_lmconv_case_reaches_its_branch(case):
    s = case.shape
    p = L.plan(*s[:5])
    print(case.id, p)
    ws = _lib.library("lmconv_bwd").ps_lmconv_bwd_workspace_bytes
    assert p.bytes == ws(*s[:5]) and tuple(p[:5]) == LM_FIGURES[case.id]
    assert LM_REACHES[case.id](p, s), case.why
    for old in L.OPERATOR_SHAPES:
        q = L.plan(*old[:5])
        assert q.bytes == ws(*old[:5])
        assert not LM_REACHES[case.id](q, old), (case.id, old)
        # the issue's five properties, on every operator shape
        assert not (q.chunk % 4 != 0 and q.chunk > 2) and not q.last < q.chunk and old[4] >= 4 and old[3] > 1 and q.N >= 8, old
    if case.id == "chunk6_short_last":
        assert p.N % 4 == 2
    elif case.id == "chunk6_d2":
        assert p.N % 4 == 3
    # no vacuous case: every gradient has a bound somewhere, on the inputs the GPU test uses
    x, m, w, b, g = L.inputs(*s[:5], seed=L.ROUTE_CASES.index(case))
    assert (m == 0).any() and ((m > 0) & (m < 1)).any() and m.shape[0] == s[0]
    assert all(bool(t.any()) for t in L.bounds(x, m, w, g, s[5])) and L.forward64(x, m, w, b, s[5])[1].any()


def test_the_lmconv_cases_are_small_and_the_operator_table_is_the_issues():
    assert sum(s[0] * (s[1] + s[2]) * s[3] * s[4] for s in (c.shape for c in L.ROUTE_CASES)) < 2e5
    got = {tuple(o[:5]): tuple(L.plan(*o[:5])[2:5]) for o in L.OPERATOR_SHAPES}
    assert got == {(3, 7, 5, 6, 9): (1, 41, 1), (2, 7, 5, 6, 9): (1, 27, 1), (2, 160, 80, 8, 8): (2, 16, 2), (2, 160, 160, 8, 8): (2, 16, 2),
                   (2, 80, 80, 8, 8): (1, 32, 1), (1, 513, 80, 8, 8): (2, 8, 2), (2, 513, 80, 8, 8): (4, 8, 4), (5, 16, 16, 32, 32): (20, 64, 20)}
    assert {p[0] for p in got.values()} == {1, 2, 4, 20}
    # the walk of the kernel, restated: from location n a lane reaches n + 4 by `j += 4; while (j >= W); while (i >= H)` on any grid
    for H, W in ((1, 1), (2, 1), (3, 3), (1, 3), (6, 9)):
        b, i, j = 0, 0, 0
        for n in range(0, 40, 4):
            assert (b, i, j) == (n // (H * W), n % (H * W) // W, n % W)
            j += 4
            while j >= W:
                j -= W
                i += 1
            while i >= H:
                i -= H
                b += 1
    assert len(L.ROUTE_CASES) == 8
