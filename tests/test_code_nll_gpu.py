"""GPU: the likelihood of given codes (csrc/code_nll.hip, pixelsynth_amd/likelihood.py, ZbufferModelPts.forward_validation) against the
fp64 definition of tests/golden/nll_ref64.py, against logits recorded from the reference, and against itself across its two layouts.

THE BOUND of the per-location comparisons is the rounding bound of the computation, not a measured number:

    |nll - nll_ref64| <= 2^-23 (2 a + 32),        |entropy - entropy_ref64| <= ln 512 * 2^-23 (2 a + 32),        a = max |x / T|

over the classes of the location.  Where it comes from, with u = 2^-24 (half an ulp, relative), y = x / T, m = max y, and
nll = log sum_k exp(y_k - m) - (y_t - m), a result of magnitude at most 2 a + ln 512:

    the division          y = x / T rounds every y by at most a u; log-sum-exp moves by at most the largest of them and y_t by its own:
                          2 a u = a 2^-23.  (The kernel divides the DIFFERENCE x_k - M, M = max x, so what it pays here is relative to
                          |y_k - m| instead: nothing for the class that carries the maximum, little for every class that matters.)
    the subtraction       y_k - m rounds by |y_k - m| u.  Inside an exponential that is a relative error of the term, and the terms weigh
                          in the logarithm of their sum with p_k: sum p_k |y_k - m| = entropy - log(sum) <= ln 512, under 7 u.  In the
                          target's own term it is up to 2 a u -- the kernel forms that term, the logarithm and the last difference in fp64.
    a 2-ulp expf          2 * 2^-23 relative in every term, so in the sum, so absolute in its logarithm: 4 u.
    a 512-term sum        of positive terms: relative (n - 1) u along the longest chain of additions, absolute in the logarithm.  A
                          straight walk over the classes would be 511 u = 255 * 2^-23 and break the bound by itself; the bound's 32 is a
                          TREE's: nine levels for 512 terms, 9 u -- which is how both kernels add (eight classes, sixteen of those, four
                          waves; or eight classes per lane and a butterfly of six levels).
    the log               of a sum in [1, 512], below 6.24: 2 ulp there are 16 u in fp32 (fp64 in the kernel).
    the final difference  rounds the fp32 result: (2 a + 6.24) u <= a 2^-23 + 4 u.

In all at most 2 a 2^-23 + (7 + 4 + 9 + 16 + 4) u = 2^-23 (2 a + 20) where the division and the target's subtraction are paid once between
them.  The kernel under test pays a 2^-23 (the last rounding) and, per class, three roundings of d = (x - M) / T (the difference, the
division, the fp32 temperature): 3 * 7 u + 4 u + 9 u + 4 u = 2^-23 * 19 -- inside 2^-23 (2 a + 32) for every a.  The entropy,
log s - (sum e d) / s with d = y - m and e = exp(d), repeats the sum with the terms weighted by |d|: the same relative errors on a mean of
|d| that is at most ln 512, and nothing in a.  The largest observed error over bound is recorded in docs/LAB_NOTEBOOK.md; above 1 the
kernel is wrong, not the bound.

`hit` is compared exactly: the arg-max is taken on the logits as they are (no division), the families keep 1e-3 between the two
largest classes except where they tie exactly, and an exact tie goes to the lowest class.
"""
import math
import os

import numpy as np
import pytest
import torch

from nll_ref64 import code_nll_ref64, rounding_bound
from pixelsynth_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F3, L = 3, 1024
LN512 = math.log(512.0)
FAMILIES = ("normal", "equal", "ahead_on", "ahead_off", "huge", "class0", "class511", "tie")


def tt(a):
    return torch.tensor(np.asarray(a), device=DEV)       # (a copy: the shared inputs are read-only arrays)


def _families(seed, F_=F3):
    """-> logits (F,L,512) f32, targets (F,L) int32, family index per location (L,): location l belongs to family l % 8"""
    rs = np.random.RandomState(seed)
    x = (3.0 * rs.randn(F_, L, 512)).astype(np.float32)
    t = rs.randint(0, 512, (F_, L)).astype(np.int32)
    fam = np.arange(L) % len(FAMILIES)
    top = x.argmax(-1)
    np.put_along_axis(x, top[..., None], np.take_along_axis(x, top[..., None], -1) + np.float32(2e-3), -1)   # a gap of >= 1e-3 at the top
    sel = lambda name: fam == FAMILIES.index(name)
    half = (np.arange(L) // len(FAMILIES)) % 2 == 0
    t[:, sel("normal") & half] = top[:, sel("normal") & half]                       # (half of the plain locations are hits)
    x[:, sel("equal")] = np.float32(1.25)
    for name in ("ahead_on", "ahead_off"):
        s = sel(name)
        lead = rs.randint(0, 512, (F_, int(s.sum())))
        xs = (0.3 * rs.randn(F_, int(s.sum()), 512)).astype(np.float32)
        np.put_along_axis(xs, lead[..., None], xs.max(-1, keepdims=True) + np.float32(80.0), -1)
        x[:, s] = xs
        t[:, s] = lead if name == "ahead_on" else (lead + 1 + rs.randint(0, 511, lead.shape)) % 512
    s = sel("huge")
    x[:, s] = np.where(rs.rand(F_, int(s.sum()), 512) < 0.5, np.float32(1e4), np.float32(-1e4))
    x[:, s, 0] = np.float32(-1e4)                                                   # (so that the lowest class at +1e4 is not always 0)
    t[:, sel("class0")] = 0
    t[:, sel("class511")] = 511
    s = sel("tie")
    pair = np.sort(np.stack([rs.choice(512, 2, replace=False) for _ in range(F_ * int(s.sum()))]).reshape(F_, -1, 2), -1)
    xs = x[:, s]
    peak = xs.max(-1, keepdims=True) + np.float32(1.0)
    np.put_along_axis(xs, pair[..., :1], peak, -1)
    np.put_along_axis(xs, pair[..., 1:], peak, -1)
    x[:, s] = xs
    t[:, s] = np.where(half[s][None], pair[..., 0], pair[..., 1])                   # on the lower class: a hit; on the upper: none
    return x, t, fam


def _regions():
    """frame 0 all observed, frame 1 all sampled, frame 2 mixed"""
    reg = np.zeros((F3, L), np.uint8)
    reg[1] = 1
    reg[2] = np.random.RandomState(8).rand(L) < 0.4
    return reg


_CASE = {}


def case(T):
    """The families, their regions and the fp64 reference at temperature T, computed once and handed out read-only"""
    if T not in _CASE:
        if "x" not in _CASE:
            x, t, fam = _families(21)
            _CASE["x"] = (x, np.ascontiguousarray(x.transpose(0, 2, 1)), t, fam, _regions())
            for a in _CASE["x"]:
                a.setflags(write=False)
        x, _, t, _, reg = _CASE["x"]
        ref = code_nll_ref64(x, t, reg, T, "lc")
        ref["bound"] = rounding_bound(x, T, "lc")
        for a in ref.values():
            a.setflags(write=False)
        _CASE[T] = ref
    return _CASE["x"] + (_CASE[T],)


def run(x, t, reg, T, layout):
    from pixelsynth_amd.likelihood import code_nll
    out = code_nll(tt(x), tt(t), None if reg is None else tt(reg), T, layout)
    torch.cuda.synchronize()
    return out


def host(r):
    return dict(nll=r.nll.cpu().numpy(), entropy=r.entropy.cpu().numpy(), hit=r.hit.cpu().numpy(), frames=r.frames.cpu().numpy())


@pytest.mark.parametrize("frames", [F3, 1])
@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("layout", ["chw", "lc"])
def test_kernel_against_the_fp64_definition(layout, T, frames):
    x_lc, x_chw, t, fam, reg, ref = case(T)
    x = (x_chw if layout == "chw" else x_lc)[:frames]
    got = host(run(x, t[:frames], reg[:frames], T, layout))
    assert got["nll"].shape == got["entropy"].shape == got["hit"].shape == (frames, L) and got["frames"].shape == (frames, 2, 4)
    assert got["nll"].dtype == got["entropy"].dtype == np.float32 and got["hit"].dtype == np.uint8
    assert np.isfinite(got["nll"]).all() and np.isfinite(got["entropy"]).all()
    bound = ref["bound"][:frames]
    e_nll = np.abs(got["nll"].astype(np.float64) - ref["nll"][:frames]) / bound
    e_ent = np.abs(got["entropy"].astype(np.float64) - ref["entropy"][:frames]) / (bound * LN512)
    for i, name in enumerate(FAMILIES):
        print(f"code_nll {layout} T={T} F={frames} {name:9s}: largest error / bound  nll {e_nll[:, fam == i].max():.4f}  "
              f"entropy {e_ent[:, fam == i].max():.4f}")
    assert e_nll.max() <= 1.0, (float(e_nll.max()), FAMILIES[fam[np.unravel_index(e_nll.argmax(), e_nll.shape)[1]]])
    assert e_ent.max() <= 1.0, (float(e_ent.max()), FAMILIES[fam[np.unravel_index(e_ent.argmax(), e_ent.shape)[1]]])
    assert np.array_equal(got["hit"], ref["hit"][:frames])
    assert 0 < got["hit"][:, fam == FAMILIES.index("tie")].mean() < 1 and got["hit"][:, fam == FAMILIES.index("ahead_on")].all()
    assert not got["hit"][:, fam == FAMILIES.index("ahead_off")].any()
    # the closed forms, through the kernel: equal logits give ln 512 twice; one class 80 ahead and the target off it gives the gap
    eq, off = fam == FAMILIES.index("equal"), fam == FAMILIES.index("ahead_off")
    assert np.abs(got["nll"][:, eq] - LN512).max() <= 2.0 ** -23 * 32 and np.abs(got["entropy"][:, eq] - LN512).max() <= 2.0 ** -23 * 32 * LN512
    gap = (x_lc[:frames].max(-1) - np.take_along_axis(x_lc[:frames], t[:frames, :, None].astype(np.int64), -1)[..., 0])[:, off].astype(np.float64) / T
    assert np.abs(got["nll"][:, off] - gap).max() <= 2.0 ** -23 * (2 * 82 / T + 32) + 512 * math.exp(-79.0)


def test_frame_table_counts_sums_and_bits():
    T = 0.7
    x_lc, x_chw, t, fam, reg, ref = case(T)
    for layout, x in (("chw", x_chw), ("lc", x_lc)):
        r = run(x, t, reg, T, layout)
        got = host(r)
        g = reg != 0
        for f in range(F3):
            for k, sel in enumerate((~g[f], g[f])):
                row = got["frames"][f, k]
                assert row[0] == sel.sum() and row[3] == got["hit"][f][sel].sum(), (layout, f, k)
                for col, name in ((1, "nll"), (2, "entropy")):
                    want = got[name][f][sel].astype(np.float64).sum()
                    assert abs(row[col] - want) <= 1e-12 * abs(want), (layout, f, k, name, row[col], want)
        assert np.array_equal(got["frames"][0, 1], np.zeros(4)) and np.array_equal(got["frames"][1, 0], np.zeros(4))   # empty groups: zeros
        assert got["frames"][2, 0, 0] > 0 and got["frames"][2, 1, 0] > 0 and got["frames"][:, :, 0].sum() == F3 * L
        # against the definition's own table: the sums of values that each keep the per-location bound
        slack = (ref["bound"] * LN512).sum(1)
        assert (np.abs(got["frames"][:, :, 1:3] - ref["frames"][:, :, 1:3]).max(axis=(1, 2)) <= slack).all()
        # a second run: the same bits
        again = host(run(x, t, reg, T, layout))
        for k in got:
            assert np.array_equal(got[k], again[k]), (layout, k)
        # a frame alone (F = 1), and at every position of the batch: its row is the same bits
        for f in range(F3):
            alone = host(run(x[f:f + 1], t[f:f + 1], reg[f:f + 1], T, layout))
            assert alone["frames"][0].tobytes() == got["frames"][f].tobytes(), (layout, f)
            assert np.array_equal(alone["nll"][0], got["nll"][f]) and np.array_equal(alone["entropy"][0], got["entropy"][f])
        perm = [2, 0, 1]
        moved = host(run(x[perm], t[perm], reg[perm], T, layout))
        assert moved["frames"].tobytes() == got["frames"][perm].tobytes(), layout
        # no region: every location observed, the sampled group empty
        bare = host(run(x, t, None, T, layout))
        assert np.array_equal(bare["frames"][:, 1], np.zeros((F3, 4))) and (bare["frames"][:, 0, 0] == L).all()
        assert np.array_equal(bare["nll"], got["nll"]) and bare["frames"][1, 0].tobytes() == got["frames"][1, 1].tobytes()
        # the result type on the device: no copy to the host, fp64 scalars
        bits = r.bits_per_code("sampled")
        assert bits.is_cuda and bits.dtype == torch.float64 and bits.dim() == 0
        want = got["frames"][:, 1, 1].sum() / got["frames"][:, 1, 0].sum() / math.log(2.0)
        assert abs(float(bits) - want) <= 1e-15 * want
        assert math.isnan(float(r.bits_per_code("sampled", per_frame=True)[0]))


@pytest.mark.parametrize("layout", ["chw", "lc"])
@pytest.mark.parametrize("n", [1, 101, 130])
def test_grids_that_do_not_fill_a_workgroup(layout, n):
    """L = 1, 101, 130: no multiple of the 64 locations of a layout-0 workgroup nor of the 4 of a layout-1 one, one and several
    workgroups per frame -- the lanes past a frame's end write nothing (the outputs lie frame after frame: a stray write would land in
    the next frame, or past the end), and the outputs can be asked for one by one."""
    from pixelsynth_amd import _lib
    T = 0.7
    x_lc, _, t, fam, reg, _ = case(T)
    x_lc, t, reg = (np.ascontiguousarray(a[:2, :n]) for a in (x_lc, t, reg))
    reg[0, ::3] = 1
    x = np.ascontiguousarray(x_lc.transpose(0, 2, 1)) if layout == "chw" else x_lc
    ref, bound = code_nll_ref64(x_lc, t, reg, T, "lc"), rounding_bound(x_lc, T, "lc")
    got = host(run(x, t, reg, T, layout))
    assert (np.abs(got["nll"] - ref["nll"]) <= bound).all() and (np.abs(got["entropy"] - ref["entropy"]) <= bound * LN512).all()
    assert np.array_equal(got["hit"], ref["hit"]) and np.array_equal(got["frames"][:, :, [0, 3]], ref["frames"][:, :, [0, 3]])
    assert (np.abs(got["frames"][:, :, 1:3] - ref["frames"][:, :, 1:3]) <= (bound * LN512).sum()).all()
    # one output at a time, the others NULL, into buffers with a guard behind them
    dx, dt = tt(x), tt(t)
    for name, dtype in (("nll", torch.float32), ("entropy", torch.float32), ("hit", torch.uint8)):
        buf = torch.full((2 * n + 64,), 7, dtype=dtype, device=DEV)
        outs = [buf if k == name else None for k in ("nll", "entropy", "hit")]
        _lib.call("ps_code_nll_f32", dx, ("chw", "lc").index(layout), dt, None, T, 2, n, *outs, None)
        back = buf.cpu().numpy()
        assert np.array_equal(back[:2 * n].reshape(2, n), got[name]), name
        assert (back[2 * n:] == 7).all(), name


@pytest.mark.parametrize("layout", ["chw", "lc"])
def test_invalid_values_stay_where_they_are(layout):
    T = 0.7
    x_lc, x_chw, t, fam, reg, ref = case(T)
    place = lambda x, f, loc, c, v: x.__setitem__((f, c, loc) if layout == "chw" else (f, loc, c), v)
    x0 = x_chw if layout == "chw" else x_lc
    base = host(run(x0, t, reg, T, layout))
    # one NaN logit: frame 2 (mixed region), a plain location of each group
    for want_group in (0, 1):
        loc = int(np.nonzero((fam == 0) & (reg[2] == want_group))[0][5])
        x = x0.copy()
        place(x, 2, loc, 37, np.float32("nan"))
        got = host(run(x, t, reg, T, layout))
        assert np.isnan(got["nll"][2, loc]) and np.isnan(got["entropy"][2, loc])
        keep = np.ones((F3, L), bool)
        keep[2, loc] = False
        for k in ("nll", "entropy", "hit"):
            assert np.array_equal(got[k][keep], base[k][keep]), (k, want_group)
        assert np.isnan(got["frames"][2, want_group, 1]) and got["frames"][2, want_group, 0] == base["frames"][2, want_group, 0]
        assert got["frames"][2, 1 - want_group].tobytes() == base["frames"][2, 1 - want_group].tobytes()
        assert got["frames"][:2].tobytes() == base["frames"][:2].tobytes()
    # one target of -1 and one of 512: never an index; NaN nll, hit 0, the distribution's entropy as it was
    t2 = t.copy()
    lo, hi = int(np.nonzero((fam == 0) & (reg[2] == 0))[0][3]), int(np.nonzero((fam == 0) & (reg[2] == 1))[0][3])
    assert base["hit"][2, lo] + base["hit"][2, hi] >= 0
    t2[2, lo], t2[2, hi] = -1, 512
    t2[0, 0] = np.iinfo(np.int32).min
    got = host(run(x0, t2, reg, T, layout))
    bad = np.zeros((F3, L), bool)
    bad[2, lo] = bad[2, hi] = bad[0, 0] = True
    assert np.isnan(got["nll"][bad]).all() and not got["hit"][bad].any()
    assert np.array_equal(got["nll"][~bad], base["nll"][~bad]) and np.array_equal(got["hit"][~bad], base["hit"][~bad])
    assert np.array_equal(got["entropy"], base["entropy"])
    assert np.isnan(got["frames"][2, 0, 1]) and np.isnan(got["frames"][2, 1, 1]) and np.isnan(got["frames"][0, 0, 1])
    assert got["frames"][1].tobytes() == base["frames"][1].tobytes()
    assert np.array_equal(got["frames"][:, :, [0, 2]], base["frames"][:, :, [0, 2]])
    assert got["frames"][2, 0, 3] == base["frames"][2, 0, 3] - base["hit"][2, lo]


def _recorded_nll(logits_cl, targets):
    """fp64 nll of recorded logits (512, n) for targets (n,) -> (nll (n,), bound (n,))"""
    x = logits_cl.T[None]
    return code_nll_ref64(x, targets[None], None, 1.0, "lc")["nll"][0], rounding_bound(x, 1.0, "lc")[0]


def test_score_codes_against_logits_recorded_from_the_reference(golden_dir):
    """The reference's own logits for given codes and masks (tests/golden/network.npz: all 512 classes at 48 recorded locations of two
    networks; tests/golden/ar_trace.npz: the logits its sample() loop saw at every fourth step, for the codes it ended with):
    score_codes on those codes and masks, per recorded location within 2 * 1e-4 -- log-softmax moves by at most twice the largest logit
    error, 1e-4 being the project's logit tolerance -- plus the rounding bound of the fp64 nll of the recorded logits; and the mean over
    the recorded locations (the sampled group of a region that marks them: autoreg_loss through the frame table) to the same tolerance."""
    from oracle import c_oracle
    from pixelsynth_amd.likelihood import score_codes
    from test_lmconv_gpu import _ar_setup, make_net, masks_for
    fx = np.load(os.path.join(golden_dir, "network.npz"))
    dmaps = dict(syn.distance_maps())
    pos = fx["positions"]
    worst = 0.0
    for wi in range(2):
        net = make_net(int(fx[f"net{wi}_wseed"]))
        order, _ = c_oracle.custom_idx(32, 32, dmaps[str(fx[f"net{wi}_order_name"])])
        masks = masks_for(order)
        codes = syn.codes(int(fx[f"net{wi}_codes_seed"]), 1)
        want, bound = _recorded_nll(fx[f"net{wi}_logits_sub"], codes.reshape(-1)[pos])
        region = np.zeros((1, 1024), np.uint8)
        region[0, pos] = 1
        r = score_codes(net, tt(codes), masks, region=tt(region))
        rep = lambda m, c: m[0:1].repeat(c, 1, 1).view(-1, 9, 1024)               # the reference's calling convention: the same result
        r2 = score_codes(net.engine(32, 32, 1), tt(codes), (rep(masks[0], 513), rep(masks[1], 160), rep(masks[2], 80)), region=tt(region))
        assert torch.equal(r.nll, r2.nll) and torch.equal(r.frames, r2.frames)
        got = r.nll.cpu().numpy()[0, pos].astype(np.float64)
        err = np.abs(got - want) / (2e-4 + bound)
        worst = max(worst, float(err.max()))
        assert err.max() <= 1.0, (wi, float(err.max()))
        assert abs(float(r.mean_nll("sampled")) - want.mean()) <= 2e-4 + bound.max(), wi
        assert float(r.sums("sampled")[0]) == len(pos)
    fx = np.load(os.path.join(golden_dir, "ar_trace.npz"))
    net = make_net(int(fx["wseed"]))
    order, region, order_loc, reg, first = _ar_setup(fx)
    final = fx["final_codes"].astype(np.int64).reshape(1, 32, 32)
    at = np.array([i * 32 + j for i, j in region])[::4]
    want, bound = _recorded_nll(fx["step_logits"].T, final.reshape(-1)[at])
    marked = np.zeros((1, 1024), np.uint8)
    marked[0, at] = 1
    r = score_codes(net, tt(final), masks_for(order), region=tt(marked))
    err = np.abs(r.nll.cpu().numpy()[0, at].astype(np.float64) - want) / (2e-4 + bound)
    worst = max(worst, float(err.max()))
    print(f"score_codes against recorded logits: largest error / (2e-4 + bound) {worst:.4f}")
    assert err.max() <= 1.0, float(err.max())
    assert abs(float(r.mean_nll("sampled")) - want.mean()) <= 2e-4 + bound.max()


def test_the_two_layouts_describe_the_same_run():
    """An AR run of three frames that keeps its logits (layout "lc": the logits every code was drawn from), and one whole-grid forward on
    the codes it ended with (layout "chw"): by the column / whole-grid invariant the logits at the sampled locations are the same bits,
    so the two scores differ by the order of the 512-term sums alone -- twice the bound."""
    from pixelsynth_amd.ar_plan import build_ar_plan
    from pixelsynth_amd.likelihood import code_nll, score_codes
    from test_lmconv_gpu import make_net
    T = 0.7
    net = make_net(3)
    bgs = syn.background_masks(256)
    plan = build_ar_plan(tt(np.stack([bgs[n] for n in ("right_half", "half_plus_island", "ragged")])), 32)
    eng = net.engine(32, 32, F3)
    codes = tt(syn.codes(11, F3).reshape(F3, L).astype(np.int32))
    u = tt(np.random.RandomState(6).rand(F3, L).astype(np.float32))
    logits = eng.ar_run(codes, plan.order_loc, plan.region, plan.mask_init, plan.mask_undilated, plan.mask_dilated, temperature=T,
                        uniforms=u, first_step=plan.first_step, want_logits=True, waves=plan.waves)
    eng.check()
    sampled = plan.region.bool()
    assert int(sampled.sum()) > 600
    # (the rows of locations no column walked are whatever the buffer held: only the sampled rows are read)
    by_loc = code_nll(torch.where(sampled[..., None], logits, torch.zeros_like(logits)), codes, plan.region, T, "lc")
    whole = score_codes(net, codes.view(F3, 32, 32), plan, temperature=T)
    full = eng.forward(codes, plan.mask_init, plan.mask_undilated, plan.mask_dilated).reshape(F3, 512, L).permute(0, 2, 1)
    assert torch.equal(full[sampled], logits[sampled])                             # the invariant this test rests on
    a, b = by_loc.nll[sampled].double().cpu().numpy(), whole.nll[sampled].double().cpu().numpy()
    assert np.isfinite(a).all() and np.isfinite(b).all()
    bound = rounding_bound(logits[sampled].cpu().numpy()[None], T, "lc")[0]
    print(f"the two layouts on one run: largest |difference| / (2 bound) nll {(np.abs(a - b) / (2 * bound)).max():.4f}")
    assert (np.abs(a - b) <= 2 * bound).all()
    ea, eb = by_loc.entropy[sampled].double().cpu().numpy(), whole.entropy[sampled].double().cpu().numpy()
    assert (np.abs(ea - eb) <= 2 * bound * LN512).all()
    assert torch.equal(by_loc.hit[sampled], whole.hit[sampled])
    assert torch.equal(by_loc.frames[:, 1, 0], whole.frames[:, 1, 0]) and torch.equal(by_loc.frames[:, 1, 3], whole.frames[:, 1, 3])
    slack = torch.from_numpy(np.array([2 * bound.sum()])).to(DEV)
    assert bool(((by_loc.frames[:, 1, 1] - whole.frames[:, 1, 1]).abs() <= slack).all())


def test_forward_validation():
    from pixelsynth_amd import driver
    from pixelsynth_amd.likelihood import score_codes
    B = 2
    model = driver.build_model(torch.device(DEV))
    model.opt.model_setting = "gen_paired_img"
    cam0 = {k: torch.from_numpy(v) for k, v in syn.demo_cameras(B).items()}
    RTinv, RT = syn.yaw_pose(syn.demo_cameras(B)["P"], 0.6)
    cam1 = dict(cam0, P=torch.from_numpy(RT), Pinv=torch.from_numpy(RTinv))
    target = torch.from_numpy(syn.image(9, B, 3, 256))
    batch = {"images": [torch.from_numpy(syn.image(4, B, 3, 256)), target], "cameras": [cam0, cam1],
             "depths": [torch.from_numpy(syn.depth_smooth(5, B, 256, 1.0, 100.0))], "codes": torch.from_numpy(syn.codes(6, B))}
    _, before = model.forward_image(batch)
    loss, out = model.forward_validation(batch)
    _, after = model.forward_image(batch)
    model.outpaint2.engine(32, 32, B).check()
    assert set(before) == set(after) and set(out) == set(before) | {"NLLMap", "EntropyMap"}
    for k in before:                                                                # no state leaks into the sampling path
        assert torch.equal(before[k], after[k]), k
    for k in ("InputImg", "PredDepthImg", "ForegroundImg", "FeaturesImg", "OutputImg"):
        assert torch.equal(out[k], before[k]), k
    assert out["PredImg"].shape == before["PredImg"].shape == (B, 3, 256, 256) and torch.equal(out["OutputImg"].cpu(), target)
    assert out["NLLMap"].shape == out["EntropyMap"].shape == (B, 1, 32, 32) and out["NLLMap"].dtype == torch.float32
    assert set(loss) == {"autoreg_loss", "ar_bits_per_code", "ar_bits_sampled", "ar_bits_observed", "ar_accuracy_sampled", "ar_frames"}
    # by hand on the same plan
    bg = ~out["ForegroundImg"][0].bool()
    assert bg.shape == (B, 256, 256) and 0.05 < float(bg.float().mean()) < 0.95
    plan = model.get_masks_for_batch(None, None, bg, compact=True)
    codes = model.vqvae.encode_codes(target.to(DEV)).reshape(B, 32, 32)
    assert torch.equal(out["PredCodes"], codes)
    want = score_codes(model, codes, plan)
    assert torch.equal(loss["autoreg_loss"], want.mean_nll("all")) and torch.equal(loss["ar_frames"], want.frames)
    assert torch.equal(out["NLLMap"].view(B, -1), want.nll) and torch.equal(out["EntropyMap"].view(B, -1), want.entropy)
    assert torch.equal(model.autoreg_score(plan, codes).nll, want.nll)
    mean = float(want.nll.double().mean())                                         # what nn.CrossEntropyLoss() returns over B * 1024 locations
    assert abs(float(loss["autoreg_loss"]) - mean) <= 1e-12 * mean and 0 < mean < 40
    ln2 = math.log(2.0)
    assert abs(float(loss["ar_bits_per_code"]) - mean / ln2) <= 1e-12 * mean
    s, o = plan.region.bool(), ~plan.region.bool()
    assert abs(float(loss["ar_bits_sampled"]) - float(want.nll[s].double().mean()) / ln2) <= 1e-12 * 40
    assert abs(float(loss["ar_bits_observed"]) - float(want.nll[o].double().mean()) / ln2) <= 1e-12 * 40
    assert abs(float(loss["ar_accuracy_sampled"]) - float(want.hit[s].double().mean())) <= 1e-15
    # the decoder sees the target's codes in the background
    assert torch.equal(out["PredImg"], model._decode_checked(out["FeaturesImg"], bg, codes.to(torch.int64)))
    assert not torch.equal(out["PredImg"], before["PredImg"])
