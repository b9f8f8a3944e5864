"""The route cases of tests/_thin_train_ref.py, checked without a GPU: every case reaches the branch of csrc/thin_train.hip it is named
for -- by the predicates that restate the kernels' own lines --, no shape of tests/test_thin_train_gpu.py reaches it already, the split the
cases rely on is the library's own (ps_thin_train_parts, ps_thin_train_workspace_bytes: host-only calls), the Functions take every case
routed through them and refuse every case routed through the entry points.  tests/test_thin_routes_gpu.py runs the same tables on the
device."""
import pytest

import _thin_train_ref as ref
from pixelsynth_amd import _lib
from pixelsynth_amd.networks import thin_train as TT


class _Old:
    """A shape of the existing tests in a Route's clothes"""

    def __init__(self, kind, frame, wide, T, k):
        self.via, self.kind, self.frame, self.wide, self.T, self.k = "function", kind, frame, wide, T, k
        self.npix = frame[0] * frame[1] * frame[2]


OLD = [_Old(*c) for c in ref.old_cases()]
FIGURES = {       # case -> (pixels, pixels of a part, parts, pixels of the last part, L)
    "capped-ragged": (266240, 1056, 253, 128, 65),
    "capped-full-in": (327680, 1280, 256, 1280, 72),
    "capped-full-out": (327680, 1280, 256, 1280, 72),
    "w96-t2": (4608, 1024, 5, 512, 64),
}


def test_the_old_tables_are_what_the_operator_tests_run():
    import itertools
    assert ref.FRAMES == [(1, 8, 64), (2, 16, 64), (3, 8, 128)] and ref.RAGGED == (5, 8, 64) and ref.WIDE == [32, 64, 128]
    assert ref.THIN_OUT == [1, 3, 4] and ref.KS == [1, 3]
    shapes = {(c.kind, c.frame, c.wide, c.T, c.k) for c in OLD}
    assert {("out",) + c for c in itertools.product(ref.FRAMES, ref.WIDE, ref.THIN_OUT, ref.KS)} <= shapes
    assert {("in", f, w, 4, k) for f, w, k in itertools.product(ref.FRAMES, ref.WIDE, ref.KS)} <= shapes
    assert {("out", (1, 64, 64), 128, 3, 3), ("in", (2, 8, 64), 64, 4, 1), ("out", (10, 8, 64), 32, 4, 3), ("out", (1, 8, 128), 32, 1, 1)} <= shapes
    assert len({r.id for r in ref.ROUTES}) == len(ref.ROUTES)


@pytest.mark.parametrize("name", sorted(ref.BRANCHES))
def test_no_old_shape_reaches_the_branch_and_a_route_does(name):
    reach = ref.BRANCHES[name]
    assert not [(c.kind, c.frame, c.wide, c.T, c.k) for c in OLD if reach(c)]
    assert [r for r in ref.ROUTES if name in r.reaches]


@pytest.mark.parametrize("route", ref.ROUTES, ids=repr)
def test_a_route_reaches_the_branches_it_is_named_for(route):
    r = route
    assert r.reaches and all(ref.BRANCHES[name](r) for name in r.reaches), [n for n in r.reaches if not ref.BRANCHES[n](r)]
    B, H, W = r.frame
    assert ref.sizes_ok(B, H, W, r.wide, r.T, r.k)
    if r.via == "function":      # the Functions take it; through the entry points alone go the shapes they refuse
        takes = TT.takes_in if r.kind == "in" else TT.takes_out
        Ci, Co = (TT.THIN_IN, r.wide) if r.kind == "in" else (r.wide, r.T)
        assert takes(Ci, Co, r.k, H, W) and (r.kind == "out" or r.T == TT.THIN_IN)
    else:
        for T in ref.ABI_T:
            for k in ref.ABI_K:
                assert not TT.takes_out(r.wide, T, k, H, W) and not TT.takes_in(T, r.wide, k, H, W), (T, k)
        assert r.via == "grad_weight" or W % ref.EX_PX == 0          # (ps_thin_expand_f32's own condition)


def test_the_figures_of_the_named_cases():
    """The walks, the splits and the chains the cases were chosen for"""
    assert [ref.walk(W) for W in (64, 128, 32, 96, 12, 20, 4, 33, 1, 2)] == [
        (32, 0), (32, 0), (0, 1), (32, 0), (8, 2), (12, 1), (0, 8), (32, 0), (0, 32), (0, 16)]
    assert [ref.carry_period(W) for W in (64, 128, 32, 96, 12, 20, 4, 33)] == [2, 4, None, 3, 3, 5, None, 33]
    assert ref.double_wrap(3, 4) and ref.double_wrap(1, 4) and not ref.double_wrap(5, 12) and not ref.double_wrap(8, 32) and not ref.double_wrap(8, 64)
    # W = 4, H = 3: from y = 2 a step of 8 rows leaves y = 10 >= 2 H, and 10 - 3 is no row -- but only a batch of more than 32 pixels has
    # a thread that takes the step: 2 x 3 x 4 has none, 4 x 3 x 4 has sixteen (pixel 32 + q after pixel q)
    assert 2 + ref.walk(4)[1] - 3 >= 3 and (2 + ref.walk(4)[1]) % 3 == 1
    assert not ref.second_step(24) and not ref.double_wrap(3, 4, 24) and ref.second_step(48) and ref.double_wrap(3, 4, 48)
    assert ref.second_step(180) and ref.second_step(231) and not ref.second_step(4) and not ref.second_step(32)
    by_id = {r.id: r for r in ref.ROUTES}
    for name, (npix, part, parts, last, L) in FIGURES.items():
        ranges = ref.part_ranges(by_id[name].npix)
        assert (by_id[name].npix, ranges[0][1] - ranges[0][0], len(ranges), ranges[-1][1] - ranges[-1][0], ref.chain(npix)) == (npix, part, parts, last, L)
    assert ref.expand_workgroups(3, 5) == [(0, 8), (8, 15)] and ref.expand_straddles(3, 5) and ref.expand_short_tail(3, 5)
    assert ref.expand_straddles(2, 24) is False and ref.expand_mod_is_no_mask(24) and not ref.expand_short_tail(2, 24)
    assert not any(ref.expand_straddles(B, H) or ref.expand_short_tail(B, H) or ref.expand_mod_is_no_mask(H) for B, H in ((1, 8), (2, 16), (3, 8), (5, 8), (1, 64)))
    assert not TT.takes_out(160, 3, 1, 16, 64) and not TT.takes_out(96, 3, 1, 16, 64) and not TT.takes_in(4, 96, 1, 16, 64)      # why those have no k = 1 case


def test_the_library_splits_the_pixels_as_the_restatement_does():
    L = _lib.library("thin_train")
    for r in ref.ROUTES:
        for T in ((r.T,) if r.via == "function" else ref.ABI_T):
            for k in ((r.k,) if r.via == "function" else ref.ABI_K):
                sizes = r.frame + (r.wide, T, k)
                assert L.ps_thin_train_parts(*sizes) == len(ref.part_ranges(r.npix)), sizes
                assert L.ps_thin_train_workspace_bytes(*sizes) == ref.workspace_bytes(*sizes), sizes
    # the boundary of the cap: 262 144 pixels are 256 parts of 1024, 32 more are 249 parts of 1056
    for frame, capped, parts in (((1, 512, 512), False, 256), ((1, 8193, 32), True, 249), ((1, 1, 262145), True, 249), ((1, 520, 512), True, 253)):
        npix = frame[0] * frame[1] * frame[2]
        assert ref.capped(npix) == capped and len(ref.part_ranges(npix)) == parts == L.ps_thin_train_parts(*frame, 32, 3, 3)
        assert L.ps_thin_train_workspace_bytes(*frame, 32, 3, 3) == ref.workspace_bytes(*frame, 32, 3, 3) == -(-parts * (27 * 32 + 64) * 4 // 256) * 256
    assert ref.part_ranges(262176)[0] == (0, 1056) and ref.part_ranges(262176)[-1] == (261888, 262176)
    assert not ref.sum_tail(262144 // 8 + 1024) and ref.sum_tail(262144) and [ref.sum_tail(n) for n in (512, 2560, 4096, 33 * 1024, 34 * 1024)] == [
        False, False, False, False, True]


def test_the_bias_shapes_reach_their_branches_and_no_old_call_does():
    old = ref.old_bias_calls()
    assert (512, 1, True) in old and (3072, 128, True) in old and (4096, 3, True) in old
    for name, reach in ref.BIAS_BRANCHES.items():
        assert not [c for c in old if reach(*c)], name
        assert [c for c, names in ref.BIAS_ROUTES if name in names], name
    for case, names in ref.BIAS_ROUTES:
        assert names and all(ref.BIAS_BRANCHES[n](*case) for n in names), case
    assert ref.bias_route(65600, 128, True) == (32, 2099200) and ref.bias_route(87400, 96, True) == (24, 2097600)
    assert ref.bias_route(699100, 3, True) == (3, 2097300) and ref.bias_route(1000, 8, False) == (8, 8000)
    assert ref.BIAS_GRID * ref.THREADS == 2097152 and not ref.bias_stride_turns(65600, 128, True)
    # the workload's own calls loop: a 256 x 256 frame of 64 channels, sixteen of them of 3
    assert ref.bias_loops(256 * 256, 64, True) is False and ref.bias_loops(16 * 256 * 256, 64, True) and ref.bias_loops(16 * 256 * 256, 3, True)
