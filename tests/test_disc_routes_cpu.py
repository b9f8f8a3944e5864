"""The route cases of the discriminator's training kernels (tests/_disc_conv_ref.py: ROUTES, BRANCHES; tests/_gan_train_ref.py:
NORM_ROUTE_CASES, FEAT_ROUTE_LISTS), checked without a GPU: every case reaches the branch of csrc/disc_conv.hip or csrc/gan_train.hip it is
there for -- by predicates that restate the kernels' own lines --, no shape of tests/test_disc_conv_gpu.py or tests/test_gan_train_gpu.py
reaches it already, the plan and the sizes the cases rely on are the library's own (host-only calls), and the operands of the exact
comparisons are exact.  tests/test_disc_routes_gpu.py runs the same tables on the device."""
import ctypes

import pytest
import torch

import _disc_conv_ref as ref
import _gan_train_ref as gref
import test_gan_train_gpu as gan_ops
from pixelsynth_amd import _lib
from pixelsynth_amd.networks import disc_conv as DC

# every shape test_disc_conv_gpu.py runs both passes at: the operator tables, a frame alone and in a batch, the overflow words, and the two
# discriminators of the network tests (ndf = 64 on a fake and a real image of 32 x 32 in one batch: maps of 17, 9, 5 and of 9, 5, 3 in front
# of model1..3; the passes on one image alone are forward passes, which the plan of the parts does not touch)
OLD = ref.ALL_SHAPES + [(3, 64, 128, 33, 34, 1), (3, 64, 128, 33, 34, 2), (1, 64, 128, 33, 34, 1), (1, 64, 128, 33, 34, 2), (2, 64, 64, 9, 11, 2)] \
    + [(2, Ci, 2 * Ci, S, S, st) for Ci, S, st in ((64, 17, 2), (128, 9, 2), (256, 5, 1), (64, 9, 2), (128, 5, 2), (256, 3, 1))]


# ---------------------------------------------------------------- the convolution
@pytest.mark.parametrize("name", sorted(ref.BRANCHES))
def test_no_old_shape_reaches_the_branch_and_a_route_does(name):
    reach = ref.BRANCHES[name]
    assert not [s for s in OLD if reach(s, ref.plan(*s))]
    assert [s for s, names in ref.ROUTES.items() if name in names]


@pytest.mark.parametrize("shape", ref.ROUTE_SHAPES, ids=str)
def test_a_route_reaches_the_branches_it_is_named_for(shape):
    p, names = ref.plan(*shape), ref.ROUTES[shape]
    assert names and all(ref.BRANCHES[n](shape, p) for n in names), [n for n in names if not ref.BRANCHES[n](shape, p)]
    assert _lib.call("ps_disc_conv_takes", *shape, 2) == 1 and DC.sizes_take(*shape)
    assert _lib.call("ps_disc_conv_parts", *shape, 2) == p.parts
    assert (p.parts - 1) * p.chunk + p.last == p.steps and 1 <= p.parts <= ref.MAX_PARTS
    total, at, part = ref.workspace_bytes(*shape)
    assert _lib.call("ps_disc_conv_workspace_bytes", *shape, 2) == total and part == p.parts * 16 * shape[1] * shape[2] * 4 and at % 256 == 0


def test_the_figures_of_the_named_cases():
    p = ref.plan(16, 64, 64, 47, 41, 1)
    assert (p.steps, p.chunk, p.parts, p.last, p.blocks) == (2304, 9, 256, 9, 2)
    assert ref.workspace_bytes(16, 64, 64, 47, 41, 1)[2] == 256 * 16 * 64 * 64 * 4               # the parts' region at 64 x 64 channels' largest
    assert 16 * 48 * 42 * 9 < 2 ** 24                                                           # the largest integer sum of grad_weight
    p = ref.plan(4, 64, 128, 129, 129, 2)
    assert (p.steps, p.chunk, p.parts, p.last, p.straddle, p.pixel_groups) == (1172, 10, 118, 2, [29, 58, 87], 17)
    assert p.launches == [(65, 65), (65, 64), (64, 65), (64, 64)]
    w = ref.plan(32, 64, 128, 129, 129, 2)                                                      # the workload's own: tools/disc_conv_time.py
    assert (w.parts, w.chunk) == (127, 74) and w.pixel_groups == p.pixel_groups and w.launches == p.launches
    p = ref.plan(1, 64, 64, 16, 5, 1)
    assert (p.steps, p.chunk, p.parts, p.last, p.odd_tail) == (9, 8, 2, 1, True)
    p = ref.plan(2, 512, 128, 9, 10, 1)
    assert (p.parts, p.straddle, p.blocks) == (3, [1], 32)
    assert [ref.plan(*s).Wo for s in ((2, 64, 64, 6, 7, 1), (1, 64, 64, 9, 15, 2))] == [8, 8]
    p = ref.plan(1, 64, 64, 3, 8, 1)
    assert (p.Wo, p.Wo8) == (9, 16)
    assert ref.plan(2, 64, 64, 1, 1, 2).launches == [(1, 1), (1, 0), (0, 1), (0, 0)]
    assert ref.plan(1, 64, 64, 1, 6, 2).launches == [(1, 3), (1, 3), (0, 3), (0, 3)]
    assert ref.plan(1, 64, 64, 4, 1, 2).launches == [(2, 1), (2, 0), (2, 1), (2, 0)]
    # Wo = 9 at stride 2 is an operator shape's already: the predicate of "wo-one-over" is about stride 1
    assert ref.plan(2, 128, 256, 17, 17, 2).Wo == 9 and not ref.BRANCHES["wo-one-over"]((2, 128, 256, 17, 17, 2), ref.plan(2, 128, 256, 17, 17, 2))
    assert set(ref.ABI_SHAPES) <= set(ref.ROUTE_SHAPES)


def test_the_scale_of_a_tiny_gradient_is_held():
    """max |g| = 3 x 2^-115 = 0.75 x 2^-113: 15 - e = 128, held at 126.  The other end, -126, would need a maximum of 2^141"""
    assert ref.scale_of(3 * 2.0 ** -115) == 2.0 ** 126 and ref.scale_of(2.0 ** -113) == 2.0 ** 126      # held: 127 and 128 asked for
    assert ref.scale_of(2.0 ** -112) == 2.0 ** 126 and ref.scale_of(2.0 ** -111) == 2.0 ** 125          # the largest not held
    assert ref.scale_of(torch.finfo(torch.float32).max) == 2.0 ** -113


def test_the_scaled_integers_are_exact():
    """x 2^8, w 2^16, g 2^-115 of the integers: operands and fp64 results survive fp32, every non-zero value a normal fp32; under the
    kernel's scales (sw = 2^-3, sg = 2^126) the split operands stay integers below 2^15, so every sum is exact"""
    x, w, g, y, gx, gw = ref.scaled_integers(ref.TINY_SHAPE, *ref.TINY_EXPONENTS)
    x0, w0, g0, y0, gx0, gw0 = ref.integers(ref.TINY_SHAPE)
    assert torch.equal(x, x0 * 2.0 ** 8) and torch.equal(w, w0 * 2.0 ** 16) and torch.equal(y, y0 * 2.0 ** 24)
    assert torch.equal(g.double(), g0.double() * 2.0 ** -115) and torch.equal(gx.double(), gx0.double() * 2.0 ** -99)
    assert torch.equal(gw.double(), gw0.double() * 2.0 ** -107)
    sg, sw = ref.scale_of(g.abs().max().item()), ref.scale_of(w.abs().max().item())
    assert (sg, sw) == (2.0 ** 126, 2.0 ** -3)
    for t, s in ((g, sg), (w, sw), (x, 1.0)):
        hi, lo = ref.split(t * s)
        assert torch.equal(hi.float(), t * s) and not lo.any() and (t * s).abs().max() < 2.0 ** 15
    tiny = torch.finfo(torch.float32).tiny
    assert all((t[t != 0].abs() >= tiny).all() for t in (g, gx, gw)) and gx.any() and gw.any()
    # the largest partial sums, times the scales, are integers below 2^24 times a power of two
    assert y0.abs().max() < 2 ** 24 and gx0.abs().max() < 2 ** 24 and gw0.abs().max() < 2 ** 24


# ---------------------------------------------------------------- the norm and the feature matching
def test_the_norm_cases_reach_the_forms_no_operator_case_does():
    old = [gref.form(s[2] * s[3]) for s in gan_ops.CASES]
    new = [gref.form(s[2] * s[3]) for s in gref.NORM_ROUTE_CASES]
    for f in gref.NORM_ROUTE_FORMS:
        assert f not in old and new.count(f) >= 2, f
    assert len(gref.NORM_ROUTE_CASES) == 20
    for b in gref.NORM_ROUTE_BOUNDARIES:
        assert gref.form(b) != gref.form(b + 1) and gref.form(b)[0] == gref.form(b + 1)[0]
        assert gref.form(b + 1)[1] == gref.form(b)[1] + 4
        planes = 5 if b + 1 <= 1793 else 2
        assert (1, planes, 1, b) in gref.NORM_ROUTE_CASES and (1, planes, 1, b + 1) in gref.NORM_ROUTE_CASES
        sizes = [s[2] * s[3] for s in gan_ops.CASES]
        assert b not in sizes and b + 1 not in sizes                 # no operator case stands on either side of the boundary
    # five planes in the wave form: the last workgroup (four planes each) has one wavefront at work
    assert all(s[1] % 4 == 1 for s in gref.NORM_ROUTE_CASES if gref.form(s[3])[0] == "wave")


def test_the_feature_lists_take_a_second_staging_trip_and_no_old_list_does():
    assert all(max(gref.feat_tiles(shapes)) <= gref.FEAT_STAGE for shapes in gan_ops.MAP_LISTS.values())
    assert gref.feat_tiles(gref.FEAT_ROUTE_LISTS["staged"]) == [258, 1, 1] and gref.feat_tiles(gref.FEAT_ROUTE_LISTS["staged-exact"]) == [512]
    assert (257 * gref.TILE + 3) % gref.TILE == 3 and 258 % gref.FEAT_STAGE == 2 and 259 % gref.FEAT_STAGE != 0
    for shapes in gref.FEAT_ROUTE_LISTS.values():
        n = len(shapes)
        halves = (ctypes.c_longlong * n)(*[s[0] * s[1] // 2 for s in shapes])
        tiles = sum(gref.feat_tiles(shapes))
        assert _lib.call("ps_gan_feat_workspace_bytes", halves, n) == -(-8 * tiles // 256) * 256


def test_the_staged_total_is_far_above_its_bound():
    """The bound discriminates: a staging trip dropped loses whole tiles of a total of about 16, against a bound of about 1e-6"""
    shapes = gref.FEAT_ROUTE_LISTS["staged"]
    maps = gref.feat_maps(shapes, seed=len(shapes))
    per, total, mag = gref.feat_forward64(maps, [5.0] * len(maps))
    bound = gref.feat_value_bound(sum(m.numel() // 2 for m in maps), mag)
    print(f"staged: total {total:.4f}, bound {bound:.3e}")
    assert 15.0 < total < 17.0 and bound < 1.5e-6 and per[0] / 258 > 1e3 * bound
