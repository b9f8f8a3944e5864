"""The route cases of tests/_norm_train_ref.py, tests/_block_train_ref.py and tests/_conv_bwd_ref.py, checked without a GPU: every case
reaches the branch of csrc/norm_train.hip, csrc/block_train.hip or csrc/conv_bwd.hip it is there for -- asserted on the Python mirrors of
the kernels' plans, whose part counts are held to the libraries' own -- and no shape of the operator tests reaches it already, so a case
that adds nothing is caught.  tests/test_train_routes_gpu.py runs the same tables on the device."""
import pytest
import torch

import _block_train_ref as B
import _conv_bwd_ref as C
import _norm_train_ref as N
from pixelsynth_amd import _lib


# ---- the norm -------------------------------------------------------------------------------------------------------------------------------
def _np(shape):
    b, c, h, w = shape
    return N.plan(b, h * w, c)


def _kinds(shape):
    b, c, h, w = shape
    return N.walk_kinds(b, h * w, c)


def _frame_batches(shape):
    p = _np(shape)
    return [N.batches(f * p.ppf, (f + 1) * p.ppf) for f in range(shape[0])]


NORM_REACHES = {       # case -> the property no operator shape has
    "chunk_tail": lambda s: _np(s).chunks > 1 and _np(s).last_cw < _np(s).cw and _np(s).fin_wgs > 1 and _np(s).last_fin < N.FIN_CH,
    "chunks_full": lambda s: _np(s).chunks > 1 and _np(s).last_cw == _np(s).cw,
    "many_frames": lambda s: len(N.batches(0, _np(s).parts)) > 1 and _np(s).parts % N.FIN_PARTS != 0,
    "many_parts_per_frame": lambda s: _np(s).ppf > N.FIN_PARTS and _np(s).ppf % N.FIN_PARTS != 0,
    "long_parts": lambda s: _np(s).part_rows > N.PART_ROWS and _np(s).parts == N.MAX_PARTS,
    "idle_lane_tails": lambda s: 0 < _np(s).idle and _np(s).cw != 48 and {("none", 0, 3), ("set0", 1, 3)} <= _kinds(s),
    "two_step_tails": lambda s: any(k[:2] == ("set1", 2) for k in _kinds(s)),
    "deep_tails": lambda s: {("set0", 3, 2), ("set0", 3, 3), ("set1", 3, 2), ("set1", 3, 3)} <= _kinds(s),
    "single_value": lambda s: s[0] * s[2] * s[3] == 1,
}


@pytest.mark.parametrize("case", N.ROUTE_CASES, ids=lambda c: c.id)
def test_norm_case_reaches_its_branch(case):
    b, c, h, w = case.shape
    hw, p, kinds = h * w, _np(case.shape), _kinds(case.shape)
    assert N.sizes_ok(b, hw, c) and p.parts == len(N.part_ranges(b, hw)) == _lib.library("norm_train").ps_norm_train_parts(b, hw, c)
    assert b * c * hw <= 1.1e6
    print(f"{case.id}: {p}, batches of all parts {[n for _, n in N.batches(0, p.parts)]}, kinds {sorted(kinds)}")
    assert NORM_REACHES[case.id](case.shape), case.why
    for shape in N.OPERATOR_SHAPES:
        assert not NORM_REACHES[case.id](shape), (case.id, shape)
    lengths = sorted({r1 - r0 for _, r0, r1 in N.part_ranges(b, hw)})
    if case.id == "chunk_tail":
        assert (p.cw, p.rl, p.idle, p.chunks, p.last_cw) == (64, 4, 0, 2, 1) and kinds == {("set0", 3, 0)} and hw == 12 * p.rl
        assert (p.fin_wgs, p.last_fin) == (9, 4)
    elif case.id == "chunks_full":
        assert (c, p.chunks, p.last_cw, p.cw) == (512, 2, 64, 64)
    elif case.id == "many_frames":
        assert p.parts == 130 and [n for _, n in N.batches(0, p.parts)] == [64, 64, 2] and p.ppf == 1
        assert p.rl > hw and ("none", 0, 0) in kinds                                   # lanes with no row
    elif case.id == "many_parts_per_frame":
        assert hw == 33280 and p.ppf == 65 and _frame_batches(case.shape) == [[(0, 64), (64, 1)], [(65, 64), (129, 1)]]
        assert 65 % N.FIN_PARTS != 0                                                     # frame 1's batches start off a multiple of 64
    elif case.id == "long_parts":
        assert hw == 1025 and p.part_rows == 1024 and p.ppf == 2 and p.parts == N.MAX_PARTS == 512
        assert [n for _, n in N.batches(0, p.parts)] == [64] * 8 and lengths == [1, 1024]
    elif case.id == "idle_lane_tails":
        assert (p.cw, p.rl, p.idle) == (3, 85, 1) and {("none", 0, 2), ("none", 0, 3), ("set0", 1, 2), ("set0", 1, 3)} <= kinds
    elif case.id == "two_step_tails":
        assert (p.cw, p.rl, p.ppf) == (5, 51, 3) and {("set0", 1, 1), ("set0", 1, 2), ("set1", 2, 2), ("set1", 2, 3)} <= kinds
    elif case.id == "deep_tails":
        assert (p.cw, p.rl, p.idle, p.ppf) == (9, 28, 4, 2) and c == 4 * p.cw


def test_the_norm_cases_take_every_exit_of_the_walk():
    """Both exits of the double-buffered loop with the fewest steps they can have (1 after set 0, 2 after set 1) and with three or
    more; every tail 0 .. 3 after a pipelined block and with none.  The operator shapes leave most of that out."""
    need_exits = {("set0", 1), ("set1", 2), ("set0", 3), ("set1", 3)}
    new = set().union(*(_kinds(c.shape) for c in N.ROUTE_CASES))
    old = set().union(*(_kinds(s) for s in N.OPERATOR_SHAPES))
    assert {k[:2] for k in new if k[0] != "none"} == need_exits
    assert {k[2] for k in new if k[0] != "none"} == {0, 1, 2, 3} == {k[2] for k in new if k[0] == "none"}
    assert ("set1", 2) not in {k[:2] for k in old} and ("none", 0, 3) not in old
    assert {k[2] for k in old if k[0] != "none"} == {0, 3} and len(new - old) >= 9
    # the restated walk at its edges: a lane with no row, one row, exactly a block, a block and a row
    assert N.walk(5, 5, 4)[:3] == ("none", 0, 0) and N.walk(9, 5, 4)[:3] == ("none", 0, 0) and N.walk(0, 1, 4)[:3] == ("none", 0, 1)
    assert N.walk(0, 13, 4)[:3] == ("set0", 1, 0) and N.walk(0, 16, 4)[:3] == ("set0", 1, 0) and N.walk(0, 17, 4)[:3] == ("set0", 1, 1)
    assert N.walk(0, 29, 4)[:3] == ("set1", 2, 0) and N.walk(0, 48, 4)[:3] == ("set0", 3, 0) and N.walk(3, 48, 4)[:3] == ("set0", 3, 0)


def test_the_wide_variance_bound_only_widens_past_2_to_the_12_rows():
    x = N.inputs(2, 4, 5, 3)[0]
    assert torch.equal(N.stat_bounds(x)[1], N.stat_bounds(x, rows=30)[1]) and torch.equal(N.stat_bounds(x)[1], N.stat_bounds(x, rows=2 ** 12)[1])
    wide, plain = N.stat_bounds(x, rows=2 ** 18)[1], N.stat_bounds(x)[1]
    m2 = N.stats64(x)[2]
    assert torch.allclose(wide - plain, (2.0 ** -34 - 2.0 ** -40) * m2, rtol=1e-12, atol=0) and torch.equal(N.stat_bounds(x)[0], N.stat_bounds(x, rows=9)[0])


# ---- the 1 x 1 convolution's weight gradient and the adjoints ---------------------------------------------------------------------------------
GW_REACHES = {       # shape -> the property no operator shape has
    (528, 128, 64): lambda p: (p.TO, p.TC) == (1, 2),
    (528, 80, 48): lambda p: (p.TO, p.TC) == (1, 2) and p.short_g and p.short_x,
    (528, 48, 80): lambda p: (p.TO, p.TC) == (2, 1) and p.short_g and p.short_x,
    (528, 192, 192): lambda p: (p.TO, p.TC) == (1, 1) and p.tiles_o > 1 and p.tiles_c > 1,
    (528, 256, 192): lambda p: (p.TO, p.TC) == (1, 2) and p.tiles_o > 1 and p.tiles_c > 1,
    (131088, 16, 16): lambda p: p.part_pix > B.MIN_PART and p.parts > 3,
}
GW_FIGURES = {       # shape -> (TO, TC, tiles_o, tiles_c, short_g, short_x, part_pix, parts, last_pix)
    (528, 128, 64): (1, 2, 1, 1, 0, 0, 512, 2, 16),
    (528, 80, 48): (1, 2, 1, 1, 48, 16, 512, 2, 16),
    (528, 48, 80): (2, 1, 1, 1, 16, 48, 512, 2, 16),
    (528, 192, 192): (1, 1, 3, 3, 0, 0, 512, 2, 16),
    (528, 256, 192): (1, 2, 3, 2, 0, 0, 512, 2, 16),
    (131088, 16, 16): (1, 1, 1, 1, 16, 16, 528, 249, 144),
}


@pytest.mark.parametrize("shape", B.GW_ROUTE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grad_weight_case_reaches_its_branch(shape):
    p = B.gw_plan(*shape)
    print(shape, p)
    assert B.sizes_ok(*shape) and p.parts == _lib.library("block_train").ps_conv1x1_grad_weight_parts(*shape)
    assert tuple(p) == GW_FIGURES[shape] and GW_REACHES[shape](p)
    assert B.gw_inputs(*shape)[0].numel() == shape[0] * shape[1]
    for old in B.GW_SHAPES:
        q = B.gw_plan(*old)
        assert not GW_REACHES[shape](q) and not q.short_g and not q.short_x and (q.TO, q.TC) != (1, 2), (shape, old)


def test_the_large_resample_shapes_take_a_second_trip_and_the_small_ones_do_not():
    total4, rest, rows = B.second_trip(B.BIG_RESAMPLE)
    assert (total4, rest, rows) == (2 ** 21 + 16384, 16384, 4) and B.BIG_RESAMPLE in B.UP_ROUTE_SHAPES and B.BIG_RESAMPLE in B.DOWN_ROUTE_SHAPES
    for s in B.UP_SHAPES + B.DOWN_SHAPES + [(1, 3, 1, 4)]:
        assert B.second_trip(s)[1] == 0
    assert all(s[2] != 1 for s in B.UP_SHAPES) and any(s[1] == 1 for s in B.UP_SHAPES) and B.UP_ROUTE_SHAPES[0][2] == 1     # W = 1 is new, H = 1 is not


@pytest.mark.parametrize("kind", ["Up", "Down"])
def test_the_closed_form_of_the_adjoints_terms_is_the_loop(kind):
    for b, h, w, c in (B.UP_SHAPES + [(1, 3, 1, 4), (1, 1, 1, 4)] if kind == "Up" else B.DOWN_SHAPES + [(1, 2, 6, 4)]):
        shape = (b, min(c, 4), h, w)
        assert torch.equal(B.adjoint_terms(kind, shape), B.adjoint_terms_loop(kind, shape)), (kind, shape)
    assert B.axis_terms("Up", 1).tolist() == [2.0] and B.axis_terms("Up", 4).tolist() == [3.0, 4.0, 4.0, 3.0]
    assert B.axis_terms("Down", 6).tolist() == [1.0, 2.0, 1.0, 2.0, 1.0, 1.0]


# ---- the 3 x 3 convolution's backward pass ---------------------------------------------------------------------------------------------------
CONV_REACHES = {
    "blocks_2x2": lambda s, p: s[3] > C.BLOCK and s[4] > C.BLOCK,
    "blocks_3x2": lambda s, p: s[3] > C.BLOCK and s[4] > 2 * C.BLOCK,
    "ragged_prep": lambda s, p: p.pchunk > C.PREP_MIN_PIXELS and p.pchunk % 16 != 0 and p.nprep == C.PREP_BLOCKS,
    "prep_scan_twice": lambda s, p: p.nprep * p.ncb > 256,
    "chunk_9": lambda s, p: p.chunk > C.MIN_CHUNK and p.straddle,
}


@pytest.mark.parametrize("case", C.ROUTE_CASES, ids=lambda c: c.id)
def test_conv_case_reaches_its_branch(case):
    s, p = case.shape, C.plan(*case.shape)
    print(case.id, p._replace(straddle=len(p.straddle)))
    L = _lib.library("conv_bwd")
    assert p.parts == L.ps_conv3x3_bwd_parts(*s) and L.ps_conv3x3_bwd_workspace_bytes(*s) >= p.parts * 9 * s[3] * s[4] * 4
    assert CONV_REACHES[case.id](s, p), case.why
    for old in C.OPERATOR_SHAPES:
        q = C.plan(*old)
        assert not CONV_REACHES[case.id](old, q), (case.id, old)
        assert q.chunk == C.MIN_CHUNK and q.pchunk == C.PREP_MIN_PIXELS and q.nprep * q.ncb <= 256 and q.nprep < C.PREP_BLOCKS
    big = max(s[0] * s[1] * s[2] * max(s[3:]), 0)
    if case.id == "blocks_2x2":
        assert p.blocks == 4 and (s[4] // C.BLOCK, s[3] // C.BLOCK) == (2, 2)
    elif case.id == "blocks_3x2":
        assert p.blocks == 6 and (s[4] // C.BLOCK, s[3] // C.BLOCK) == (3, 2)
    elif case.id == "ragged_prep":
        assert (p.pchunk, p.nprep, p.parts, p.last, p.chunk) == (75, 256, 38, 4, 8)
    elif case.id == "prep_scan_twice":
        assert p.nprep * p.ncb == 512 and p.pchunk == 75
    elif case.id == "chunk_9":
        assert (p.chunk, p.parts, p.per_frame, p.pchunk, p.nprep) == (9, 243, 728, 546, 256) and p.per_frame % p.chunk != 0
        assert len(p.straddle) == 2 and 8.9e6 < big < 9.0e6
    assert sum(1 for c in C.ROUTE_CASES if c.shape[0] * c.shape[1] * c.shape[2] > 10 ** 5) == 1          # the only case of its size
