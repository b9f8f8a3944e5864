"""GPU: the overflow guard of the split-fp16 convolutions (ps_conv3x3_f16x3_ex_nhwc, ps_conv3x3_thin_in_f16x3_nhwc) and what the plain
fp32 kernels do with a NaN.

networks/f16x3.py, DESIGN.md and the kernels' headers promise the flag for "|v| > 65000, or not a number" of the ACTIVATED value.  Under
the fused norm + ReLU the value used to pass through max(v * scale - shift, 0) first, and max() is IEEE maxNum (v_max_f32): a NaN came
out as 0, the flag stayed clear and the output was finite -- a clean-looking image from a broken input, where the fp32 route and the
reference give NaN.  The kernels now activate with ps::relu_keep_nan (v < 0 ? 0 : v).  The offending value is placed wherever a staging
path of its own reads it: an interior pixel, a corner pixel (halo and one tile only), the last chunk of three, a frame that is some
workgroup's THIRD item (fetched and stashed inside the walk, chosen on the mirror), under space-to-depth; and in scale / shift
themselves.  What is legal stays legal: a huge negative value in front of the ReLU, -inf, 65000 exactly, every channel just under it.

The fp32 kernels that carry the same max() stand in for torch ops that propagate a NaN and have no flag: their outputs' isnan masks are
held against the torch ops in fp64.
"""
import warnings

import pytest
import torch

import _conv_f16x3_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")


def _f16x3_flag(x, w, sc=None, sh=None, **kw):
    y, flag = M.run(x, M.pack(w), w.shape[0], sc, sh, **kw)
    return int(flag.item()), y


def _thin(x, w, sc=None, sh=None):
    """ps_conv3x3_thin_in_f16x3_nhwc on x (B, 4, H, W), w (64, 4, 3, 3) -> (y NCHW view, flag)"""
    from pixelsynth_amd import _lib
    B, _, H, W = x.shape
    xl, wl = x.permute(0, 2, 3, 1).contiguous(), w.permute(2, 3, 1, 0).contiguous()
    y = torch.full((B, H, W, 64), NAN, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.call("ps_conv3x3_thin_in_f16x3_nhwc", xl, sc, sh, wl, B, H, W, 64, y, flag)
    return y.permute(0, 3, 1, 2), int(flag.item())


def _ones(B, C):
    return torch.ones(B, C, device=DEV), torch.zeros(B, C, device=DEV)


# ---- where the offending value sits: (name, builder -> (x, w, kwargs, index of the offending element of x)) ------------------------------
def _place(where):
    g = torch.Generator().manual_seed(len(where))
    kw = {}
    if where == "interior":                     # B = 1, 32 x 32 (2 x 2 tiles), Ci = 32: pixel (9, 20) lies inside one tile
        B, Ci, H, at = 1, 32, 32, (0, 5, 9, 20)
    elif where == "corner":                     # pixel (31, 31): the last tile's own corner, read by that tile alone and by no halo
        B, Ci, H, at = 1, 32, 32, (0, 3, 31, 31)
    elif where == "last chunk":                 # Ci = 96: channel 95 is fetched as chunk 2, two stashes after the prologue's
        B, Ci, H, at = 1, 96, 16, (0, 95, 4, 4)
    elif where == "third item":                 # the smallest batch with a three-item walk; a frame that is the third item of a workgroup
        B, _ = M.smallest_batch(lambda p: p["longest"] >= 3, 64, 64, 128)
        frames = M.nth_item_frames(M.device_launch(B, 64, 64, 128), 2)
        assert frames, "no workgroup of this launch walks three items"
        ln = M.device_launch(B, 64, 64, 128)
        it = next(w[2] for w in M.walks(ln) if len(w) > 2 and w[2].b == frames[-1])
        Ci, H, at = 32, 64, (it.b, 7, it.ty + 5, it.tx + 6)          # inside that very item's tile
    elif where == "s2d":                        # real x (1, 32, 64, 64) read as (1, 128, 32, 32): sub-position (1, 0) = chunk 2
        B, Ci, H, at = 1, 32, 64, (0, 9, 21, 40)
        kw = dict(in_s2d=True)
    x = torch.randn(B, Ci, H, H, generator=g).to(DEV)
    Cw = 4 * Ci if kw else Ci
    w = (torch.randn(128, Cw, 3, 3, generator=g) / (3 * Cw ** 0.5)).to(DEV)
    return x, w, kw, at


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("where", ["interior", "corner", "last chunk", "third item", "s2d"])
def test_f16x3_flags_one_value_fp16_cannot_hold_wherever_it_is_staged(where, fuse):
    """One offending activation -- NaN, +inf, and unfused +-7e4 -- at each place; the flag must be 1.  Clean input first: the flag is 0.
    Fused: scale 1, shift 0 (the identity in front of the ReLU), so the ReLU alone stands between the value and the guard."""
    x, w, kw, at = _place(where)
    Cs = x.shape[1] * (4 if kw else 1)
    sc, sh = _ones(x.shape[0], Cs) if fuse else (None, None)
    assert _f16x3_flag(x, w, sc, sh, **kw)[0] == 0
    for bad in (NAN, INF) if fuse else (NAN, INF, 7e4, -7e4):
        xb = x.clone()
        xb[at] = bad
        assert _f16x3_flag(xb, w, sc, sh, **kw)[0] == 1, f"{where}, fused {fuse}: {bad} at {at} did not raise the flag"


@pytest.mark.parametrize("what", ["beyond the range after the affine", "nan in scale", "nan in shift", "inf times scale 0"])
def test_f16x3_flags_what_the_fused_affine_makes(what):
    """x = 100 under scale 1e3 is 1e5 when it reaches the split; a NaN in scale or shift makes a whole channel NaN; inf * 0 is NaN."""
    x, w, kw, at = _place("interior")
    sc, sh = _ones(1, 32)
    assert _f16x3_flag(x, w, sc, sh)[0] == 0
    if what == "beyond the range after the affine":
        x[at], sc[0, at[1]] = 100.0, 1e3
    elif what == "nan in scale":
        sc[0, 17] = NAN
    elif what == "nan in shift":
        sh[0, 30] = NAN
    else:
        x[at], sc[0, at[1]] = INF, 0.0
    assert _f16x3_flag(x, w, sc, sh)[0] == 1


@pytest.mark.parametrize("what", ["-1e30 under the relu", "-inf under the relu", "65000 exactly", "65000 exactly, fused", "every channel just under 6.5e4"])
def test_f16x3_keeps_clear_for_what_is_legal(what):
    """The flag stays 0 and the result is held to the walk tests' measure (tests/_conv_f16x3_ref.py): B = 2, 32 x 32, Ci = 32, Co = 128.
    The ReLU zeroes a huge negative value and -inf before the guard sees them; 65000 is the last value the guard lets through; a tensor
    whose every value is within 64000 .. 64990 in magnitude, either sign, is legal."""
    g = torch.Generator().manual_seed(5)
    B, Ci, H = 2, 32, 32
    x = torch.randn(B, Ci, H, H, generator=g)
    w = (torch.randn(128, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)).to(DEV)
    fuse = "relu" in what or "fused" in what
    if what == "-1e30 under the relu":
        x[0, 3, 9, 20] = x[1, 31, 0, 0] = -1e30
    elif what == "-inf under the relu":
        x[0, 3, 9, 20] = x[1, 31, 0, 0] = -INF
    elif what.startswith("65000 exactly"):
        x[0, 3, 9, 20] = x[1, 31, 0, 0] = 65000.0
        if not fuse:
            x[1, 0, 31, 31] = -65000.0
    else:
        x = (64000.0 + 990.0 * torch.rand(B, Ci, H, H, generator=g)) * (1 - 2 * torch.randint(0, 2, (B, Ci, H, H), generator=g))
    x = x.to(DEV)
    sc, sh = _ones(B, Ci) if fuse else (None, None)
    flag, y = _f16x3_flag(x, w, sc, sh)
    assert flag == 0
    M.hold(y, M.reference(M.activated(x, sc, sh), w), what)


@pytest.mark.parametrize("fuse", [True, False])
def test_thin_in_f16x3_flags_and_keeps_clear(fuse):
    """ps_conv3x3_thin_in_f16x3_nhwc (4 -> 64, B = 2, 8 x 32): the same guard.  An interior pixel and a corner pixel; fused also the
    affine's own products; the legal cases stay clear, with the result held to the same measure (K = 36 products per output)."""
    g = torch.Generator().manual_seed(9)
    B, H, W = 2, 8, 32
    x = torch.randn(B, 4, H, W, generator=g).to(DEV)
    w = (torch.randn(64, 4, 3, 3, generator=g) / 6).to(DEV)
    sc, sh = _ones(B, 4) if fuse else (None, None)
    y, flag = _thin(x, w, sc, sh)
    assert flag == 0
    M.hold(y, M.reference(M.activated(x, sc, sh), w), f"thin_in fused {fuse}")
    for at in ((1, 2, 4, 17), (0, 0, 0, 0), (1, 3, 7, 31)):
        for bad in (NAN, INF) if fuse else (NAN, INF, 7e4, -7e4):
            xb = x.clone()
            xb[at] = bad
            assert _thin(xb, w, sc, sh)[1] == 1, f"thin_in, fused {fuse}: {bad} at {at} did not raise the flag"
    if fuse:
        for what in ("beyond", "nan in scale", "nan in shift", "inf times 0"):
            xb, s1, s2 = x.clone(), sc.clone(), sh.clone()
            if what == "beyond":
                xb[1, 2, 4, 17], s1[1, 2] = 100.0, 1e3
            elif what == "nan in scale":
                s1[0, 1] = NAN
            elif what == "nan in shift":
                s2[1, 3] = NAN
            else:
                xb[1, 2, 4, 17], s1[1, 2] = INF, 0.0
            assert _thin(xb, w, s1, s2)[1] == 1, f"thin_in: {what} did not raise the flag"
    legal = [("65000 exactly", 65000.0)] + ([("-1e30 under the relu", -1e30), ("-inf under the relu", -INF)] if fuse else [("-65000 exactly", -65000.0)])
    for what, v in legal:
        xb = x.clone()
        xb[1, 2, 4, 17] = xb[0, 0, 0, 0] = v
        y, flag = _thin(xb, w, sc, sh)
        assert flag == 0, what
        M.hold(y, M.reference(M.activated(xb, sc, sh), w), f"thin_in {what}")
    xb = ((64000.0 + 990.0 * torch.rand(B, 4, H, W, generator=g)) * (1 - 2 * torch.randint(0, 2, (B, 4, H, W), generator=g))).to(DEV)
    y, flag = _thin(xb, w, sc, sh)
    assert flag == 0
    M.hold(y, M.reference(M.activated(xb, sc, sh), w), "thin_in every channel just under 6.5e4")


def test_checked_reruns_a_fused_nan_in_fp32():
    """f16x3.checked(device, fn) around a conv3x3 of a pack3x3 layer whose fused input holds a NaN: the flag is raised, checked() warns
    and runs fn again under decoder_conv("fp32"); what comes back has exactly the NaNs of torch's conv2d(relu(x * scale - shift))."""
    from pixelsynth_amd.networks import f16x3
    g = torch.Generator().manual_seed(3)
    B, Ci, Co, H = 2, 32, 64, 32
    x = torch.randn(B, Ci, H, H, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    x[1, 4, 10, 10] = NAN
    w, b = (torch.randn(Co, Ci, 3, 3, generator=g) * 0.05).to(DEV), torch.randn(Co, generator=g).to(DEV)
    sc, sh = (torch.rand(B, Ci, generator=g) + 0.5).to(DEV), (torch.randn(B, Ci, generator=g) * 0.3).to(DEV)
    p = f16x3.pack3x3(w, b)
    modes = []

    def fn():
        modes.append(f16x3.forced_mode())
        if f16x3.forced_mode() == "fp32":
            return torch.nn.functional.conv2d(M.activated(x, sc, sh), w, b, 1, 1)
        return f16x3.conv3x3(x, p, sc, sh)
    with pytest.warns(UserWarning, match="fp16's range"):
        out = f16x3.checked(x.device, fn)
    assert modes == [None, "fp32"]
    want = torch.nn.functional.conv2d(M.activated(x, sc, sh).double(), w.double(), b.double(), 1, 1)
    assert torch.equal(torch.isnan(out), torch.isnan(want)) and int(torch.isnan(want).sum()) == 9 * Co
    x[1, 4, 10, 10] = 0.5                                   # the same call on a clean input: one run, no warning
    del modes[:]
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*fp16's range.*")
        f16x3.checked(x.device, fn)
    assert modes == [None]


# ---- the fp32 kernels with the same max(): no flag, so a NaN has to come out where torch's op puts it -----------------------------------
def _affine_relu(x):
    from pixelsynth_amd import _lib
    B, C, H, W = x.shape
    g = torch.Generator().manual_seed(1)
    sc, sh = (torch.rand(B, C, generator=g) + 0.5).to(DEV), torch.randn(B, C, generator=g).to(DEV)
    y = torch.empty(B, H, W, C, device=DEV)
    _lib.call("ps_affine_relu_nhwc_f32", x.permute(0, 2, 3, 1).contiguous(), sc, sh, B, H * W, C, y)
    return y.permute(0, 3, 1, 2), torch.relu(x.double() * sc.double().view(B, C, 1, 1) - sh.double().view(B, C, 1, 1))


def _thin_f32(Co):
    def run(x):
        from pixelsynth_amd import _lib
        B, C, H, W = x.shape
        g = torch.Generator().manual_seed(2)
        sc, sh = (torch.rand(B, C, generator=g) + 0.5).to(DEV), torch.randn(B, C, generator=g).to(DEV)
        w = (torch.randn(Co, C, 3, 3, generator=g) * 0.1).to(DEV)
        y = torch.empty(B, H, W, Co, device=DEV)
        xl, wl = x.permute(0, 2, 3, 1).contiguous(), w.permute(2, 3, 1, 0).contiguous()
        if C == 4:
            _lib.call("ps_conv3x3_thin_in_nhwc_f32", xl, sc, sh, wl, B, H, W, Co, y)
        else:
            _lib.call("ps_conv3x3_thin_out_nhwc_f32", xl, sc, sh, wl, B, H, W, C, Co, y)
        xa = torch.relu(x.double() * sc.double().view(B, C, 1, 1) - sh.double().view(B, C, 1, 1))
        return y.permute(0, 3, 1, 2), torch.nn.functional.conv2d(xa, w.double(), None, 1, 1)
    return run


def _conv1x1(Co, bad_res):
    def run(x):
        """flags 3: max(x, 0) on the way in, max(res, 0) on the way out; bad_res: the NaN / inf sits in res instead of x"""
        from pixelsynth_amd import _lib
        B, C, H, W = x.shape
        g = torch.Generator().manual_seed(3)
        w = (torch.randn(Co, C, generator=g) / C ** 0.5).to(DEV)
        bias = torch.randn(Co, generator=g).to(DEV)
        clean = torch.randn(B, C, H, W, generator=g).to(DEV)
        res = torch.randn(B, Co, H, W, generator=g).to(DEV)
        if bad_res:                                   # move the offending values from x into res (same pixels, channel modulo Co)
            bad = ~torch.isfinite(x)
            for b, c, i, j in bad.nonzero().tolist():
                res[b, c % Co, i, j] = x[b, c, i, j]
            x = clean
        assert _lib.call("ps_conv1x1_takes", C, Co) == 1
        y = torch.empty(B, H, W, Co, device=DEV)
        _lib.call("ps_conv1x1_ex_nhwc_f32", x.permute(0, 2, 3, 1).contiguous(), C, w, bias, res.permute(0, 2, 3, 1).contiguous(), 3, B * H * W, C, Co, y)
        want = torch.nn.functional.conv2d(torch.relu(x.double()), w.double().view(Co, C, 1, 1), bias.double()) + torch.relu(res.double())
        return y.permute(0, 3, 1, 2), want
    return run


def _vq_head(x):
    from pixelsynth_amd import _lib
    B, C, H, W = x.shape
    g = torch.Generator().manual_seed(4)
    wt, bias = (torch.randn(64, 3, 4, 4, generator=g) * 0.1).to(DEV), torch.randn(3, generator=g).to(DEV)
    y = torch.empty(B, 3, 2 * H, 2 * W, device=DEV)
    _lib.call("ps_vq_head_f32", x.permute(0, 2, 3, 1).contiguous(), wt, bias, B, H, W, y)
    return y, torch.nn.functional.conv_transpose2d(torch.relu(x.double()), wt.double(), bias.double(), 2, 1)


@pytest.mark.parametrize("name,C,H,W,kernel", [
    ("affine_relu", 8, 6, 10, _affine_relu),
    ("thin_in 4 -> 8", 4, 8, 64, _thin_f32(8)),
    ("thin_out 32 -> 3", 32, 8, 32, _thin_f32(3)),
    ("conv1x1 64 -> 128, x", 64, 5, 7, _conv1x1(128, False)),            # 16-channel chunks, vector stores
    ("conv1x1 64 -> 128, res", 64, 5, 7, _conv1x1(128, True)),
    ("conv1x1 4 -> 64, x", 4, 5, 7, _conv1x1(64, False)),                # the four-channel form
    ("conv1x1 128 -> 3, res", 128, 5, 7, _conv1x1(3, True)),             # scalar stores
    ("conv1x1 128 -> 3, x", 128, 5, 7, _conv1x1(3, False)),
    ("vq_head", 64, 6, 16, _vq_head),
])
def test_fp32_kernels_put_a_nan_where_torch_puts_it(name, C, H, W, kernel):
    """ps_affine_relu_nhwc_f32, the fused inputs of ps_conv3x3_thin_in / thin_out_nhwc_f32, relu_in / relu_res of ps_conv1x1_ex_nhwc_f32
    and the ReLU of ps_vq_head_f32: a NaN and a +inf in the input (B = 2; an interior pixel of frame 0, the last pixel of frame 1), the
    output's isnan mask against the torch ops they replace, in fp64.  (+inf is legal fp32: it must come out as +-inf, not as NaN.)"""
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(2, C, H, W, generator=g).to(DEV)
    got, want = kernel(x)
    assert not torch.isnan(got).any() and not torch.isnan(want).any()
    x[0, C // 2, 2, 3] = NAN
    x[1, C - 1, H - 1, W - 1] = INF
    got, want = kernel(x)
    assert torch.isnan(want).any()
    ours, theirs = torch.isnan(got), torch.isnan(want)
    assert torch.equal(ours, theirs), f"{name}: {int((ours & ~theirs).sum())} NaNs torch does not have, {int((theirs & ~ours).sum())} of torch's missing"
