"""CPU-only: the host side of the locally masked convolution's backward pass (csrc/lmconv_bwd.hip, lmconv/locally_masked_convolution.py,
likelihood.ar_loss): the C ABI of libpixelsynth_lmconv_bwd.so against its header and bindings, its refusals before anything is launched,
the fp64 formulas and bounds of tests/_lmconv_bwd_ref.py against torch autograd, and the front ends' refusal of CPU tensors."""
import os
import re

import pytest
import torch

import _lmconv_bwd_ref as ref
from abi_util import ROOT, assert_library_matches_header
from oracle import lmconv_oracle as lo
from pixelsynth_amd import _lib, _libraries, likelihood
from pixelsynth_amd.lmconv.locally_masked_convolution import _locally_masked_conv2d, locally_masked_conv2d


def test_the_registry_has_the_lmconv_bwd_library():
    entry = next(e for e in _libraries.LIBRARIES if e.name == "lmconv_bwd")
    assert entry.so == "libpixelsynth_lmconv_bwd.so" and entry.headers == ("pixelsynth_lmconv_bwd.h",)
    assert entry.last_error == "ps_lmconv_bwd_last_error"
    assert [u for u, _ in entry.units] == ["lmconv_bwd.hip"] and entry.units[0][1] == _libraries.NO_CONTRACT
    protos = assert_library_matches_header("lmconv_bwd")
    assert set(protos) == set(_lib.LMCONV_BWD_PROTOS) == {"ps_lmconv_bwd_last_error", "ps_lmconv_bwd_workspace_bytes",
                                                          "ps_lmconv_grad_weight_f32", "ps_lmconv_adjoint_mask_f32"}
    # the constant the tests' bound is made of is the header's
    header = open(os.path.join(ROOT, "include", "pixelsynth_lmconv_bwd.h")).read()
    assert int(re.search(r"#define PS_LMCONV_BWD_MAX_PARTS (\d+)", header).group(1)) == ref.MAX_PARTS == 64
    # the pinned library does not export what this one adds
    assert not any(hasattr(_lib.lib(), fn) for fn in protos)


def test_workspace_bytes():
    ws = _lib.library("lmconv_bwd").ps_lmconv_bwd_workspace_bytes
    for args in ((0, 7, 5, 6, 9), (3, 0, 5, 6, 9), (3, 7, -1, 6, 9), (3, 7, 5, 0, 9), (3, 7, 5, 6, 0), (1 << 15, 7, 5, 1 << 8, 1 << 8)):
        assert ws(*args) == 0, args
    # channels-last copies of g and x padded to 16 channels, and at least one part of nine padded tiles
    B, Ci, Co, H, W = 3, 7, 5, 6, 9
    n = B * H * W
    least = 4 * (n * 16 + n * 16 + 9 * 16 * 16)
    assert least <= ws(B, Ci, Co, H, W) <= 4 * (n * 16 + n * 16 + ref.MAX_PARTS * 9 * 16 * 16) + 3 * 256
    assert ws(B, Ci, Co, H, W) % 256 == 0
    # a 160 -> 160 layer at B = 16, 32 x 32: the split keeps the partial tiles far below one part per location step
    big = ws(16, 160, 160, 32, 32)
    assert 4 * 2 * 16384 * 160 < big <= 4 * (2 * 16384 * 160 + ref.MAX_PARTS * 9 * 160 * 160) + 3 * 256


def test_entry_points_refuse_before_anything_is_launched():
    L = _lib.library("lmconv_bwd")
    err = L.ps_lmconv_bwd_last_error
    p = torch.zeros(64).data_ptr()                     # (any aligned non-null address: the arguments are refused before it is looked at)
    B, Ci, Co, H, W = 3, 7, 5, 6, 9
    need = L.ps_lmconv_bwd_workspace_bytes(B, Ci, Co, H, W)
    gw = lambda *a: L.ps_lmconv_grad_weight_f32(*a, None)
    ok = [p, p, p, 0, B, Ci, Co, H, W, 1, p, p, p, need]
    def bad(**kw):
        names = ["x", "g", "mask", "stride", "B", "Ci", "Co", "H", "W", "dil", "gw", "gb", "ws", "bytes"]
        return [kw.get(n, v) for n, v in zip(names, ok)]
    assert gw(*bad(g=None)) != 0 and b"null pointer" in err()
    assert gw(*bad(x=None)) != 0 and b"null pointer" in err()
    assert gw(*bad(mask=None)) != 0 and b"null pointer" in err()
    assert gw(*bad(ws=None)) != 0 and b"null pointer" in err()
    assert gw(*bad(gw=None, gb=None)) != 0 and b"no output" in err()
    for name in ("B", "Ci", "Co", "H", "W"):
        for v in (0, -3):
            assert gw(*bad(**{name: v})) != 0 and f"{name} = {v}".encode() in err(), (name, v)
    assert gw(*bad(dil=0)) != 0 and b"dilation = 0" in err()
    assert gw(*bad(stride=5)) != 0 and b"mask_batch_stride = 5" in err()
    assert gw(*bad(bytes=need - 1)) != 0 and b"workspace of" in err() and str(need).encode() in err()
    assert gw(*bad(bytes=0)) != 0 and b"workspace of 0 bytes" in err()
    assert gw(*bad(ws=p + 4)) != 0 and b"aligned to 16 bytes" in err()
    assert gw(*bad(B=1 << 15, H=1 << 8, W=1 << 8)) != 0 and b"locations" in err()
    adj = lambda *a: L.ps_lmconv_adjoint_mask_f32(*a, None)
    assert adj(None, 1, H, W, 1, p) != 0 and b"null pointer" in err()
    assert adj(p, 1, H, W, 1, None) != 0 and b"null pointer" in err()
    assert adj(p, 1, H, W, 1, p) != 0 and b"in place" in err()
    q = p + 128
    assert adj(p, 0, H, W, 1, q) != 0 and b"Bm = 0" in err()
    assert adj(p, 1, -1, W, 1, q) != 0 and b"H = -1" in err()
    assert adj(p, 1, H, 0, 1, q) != 0 and b"W = 0" in err()
    assert adj(p, 1, H, W, 0, q) != 0 and b"dilation = 0" in err()
    assert adj(p, 1 << 15, 1 << 8, 1 << 8, 1, q) != 0 and b"locations" in err()
    # through the binding: a CPU tensor is refused by name before a stream is looked up
    with pytest.raises(RuntimeError, match=r"ps_lmconv_adjoint_mask_f32: args\[0\] is a CPU tensor.*no CPU fallback"):
        _lib.call("ps_lmconv_adjoint_mask_f32", torch.zeros(1, 9, 4), 1, 2, 2, 1, torch.zeros(1, 9, 4))


CASES = [  # B, Ci, Co, H, W, dilation, masks, fractional
    (3, 7, 5, 6, 9, 2, 1, False), (2, 7, 5, 6, 9, 1, 2, True), (2, 4, 3, 3, 2, 2, 2, True), (1, 3, 2, 1, 5, 1, 1, False)]


def _inputs(B, Ci, Co, H, W, Bm, frac, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Ci, H, W, generator=gen)
    w = torch.randn(Co, Ci, 3, 3, generator=gen) * 0.1
    b = torch.randn(Co, generator=gen)
    m = torch.rand(Bm, 9, H * W, generator=gen)
    m = torch.where(m < 0.4, torch.zeros_like(m), m if frac else torch.ones_like(m))
    g = torch.randn(B, Co, H, W, generator=gen)
    return x, m, w, b, g


@pytest.mark.parametrize("B,Ci,Co,H,W,dil,Bm,frac", CASES)
def test_adjoint_identity_and_bounds_against_fp64_autograd(B, Ci, Co, H, W, dil, Bm, frac):
    x, m, w, b, g = _inputs(B, Ci, Co, H, W, Bm, frac)
    gx, gw, gb = ref.gradients(x, m, w, b, g, dil)
    # grad_x is the masked convolution of g with the adjoint mask and the flipped, transposed weight
    via = lo.lmconv(g.double(), ref.adjoint_mask(m.double(), H, W, dil), ref.adjoint_weight(w.double()), None, dil)
    assert (via - gx).abs().max() <= 1e-12 * max(1.0, float(gx.abs().max()))
    # the definition, element by element, on one entry of each
    o, c, t = Co - 1, Ci - 1, 2
    xpad = torch.nn.functional.pad(x.double(), (dil, dil, dil, dil))
    di, dj = (t // 3 - 1) * dil, (t % 3 - 1) * dil
    shifted = xpad[:, c, dil + di:dil + di + H, dil + dj:dil + dj + W].reshape(B, H * W)
    want = (g.double()[:, o].reshape(B, H * W) * m.double()[:, t].expand(B, -1) * shifted).sum()
    assert abs(float(gw[o, c, t // 3, t % 3] - want)) <= 1e-12 * max(1.0, abs(float(want)))
    assert (gb - g.double().sum((0, 2, 3))).abs().max() <= 1e-12
    # the bounds hold torch's own fp32 backward, and a dropped term does not pass them
    bx, bw, bb = ref.bounds(x, m, w, g, dil)
    fx, fw, fb = ref.gradients(x, m, w, b, g, dil, torch.float32)
    assert ref.check("torch fp32 grad_x", fx, gx, bx) <= 1.0 and ref.check("torch fp32 grad_w", fw, gw, bw) <= 1.0
    assert ref.check("torch fp32 grad_bias", fb, gb, bb) <= 1.0
    g2 = g.clone()
    g2[0, :, 0, 0] = 0                                 # the terms of one location dropped
    dx, dw, db = ref.gradients(x, m, w, b, g2, dil)
    assert ref.ratio(dw, gw, bw) > 1.0 and ref.ratio(db, gb, bb) > 1.0 and ref.ratio(dx, gx, bx) > 1.0
    # the repeated form of the mask, (B*Ci,9,L), is the same function
    rep = m.expand(B, -1, -1).unsqueeze(1).repeat(1, Ci, 1, 1).reshape(B * Ci, 9, H * W)
    for a, b_ in zip(ref.gradients(x, rep, w, b, g, dil), (gx, gw, gb)):
        assert torch.equal(a, b_)


def test_ratio_wants_exact_zeros_where_the_bound_is_zero():
    want, bound = torch.zeros(3, dtype=torch.float64), torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    assert ref.ratio(torch.tensor([0.0, 0.5, 0.0]), want, bound) == 0.5
    with pytest.raises(AssertionError, match="exactly 0"):
        ref.ratio(torch.tensor([0.0, 0.5, 1e-30]), want, bound)
    H, W = 3, 4
    m = torch.arange(1.0, 9 * H * W + 1).reshape(1, 9, H * W)
    a = ref.adjoint_mask(m, H, W, 2)
    assert a[0, 4].equal(m[0, 4]) and a[0, 0, 0] == 0 and a[0, 8, 0] == m[0, 0, 2 * W + 2] and a[0, 0, 2 * W + 2] == m[0, 8, 0]
    assert int((a != 0).sum()) == sum(max(0, H - abs(t // 3 - 1) * 2) * max(0, W - abs(t % 3 - 1) * 2) for t in range(9))


def test_front_ends_refuse_cpu_tensors_and_what_the_reference_refuses():
    conv = locally_masked_conv2d(4, 6)
    x, m = torch.zeros(1, 4, 5, 5, requires_grad=True), torch.ones(1, 9, 25)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(x, m)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(x, m)
    assert issubclass(_locally_masked_conv2d, torch.autograd.Function)
    with pytest.raises(NotImplementedError, match="conv_mask_weight"):
        _locally_masked_conv2d.apply(x, m, conv.weight, torch.ones(6, 3, 3), conv.bias, 1, 1)
    with pytest.raises(AssertionError, match="mask takes no gradient"):
        _locally_masked_conv2d.apply(x, m.clone().requires_grad_(), conv.weight, None, conv.bias, 1, 1)
    from pixelsynth_amd.lmconv.layers import PONO
    from pixelsynth_amd.lmconv.model import OurPixelCNN
    net = OurPixelCNN(nr_resnet=1, nr_filters=8, input_channels=512, kernel_size=(3, 3), max_dilation=2, weight_norm=False,
                      feature_norm_op=lambda c: PONO(), dropout_prob=0, conv_bias=True)
    codes = torch.zeros(1, 2, 2, dtype=torch.int64)
    masks = (torch.ones(1, 9, 4),) * 3
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        likelihood.ar_loss(net, codes, masks)
    with pytest.raises(ValueError, match="group is 'background'"):
        likelihood.ar_loss(net, codes, masks, group="background")
    with pytest.raises(ValueError, match="temperature = 0"):
        likelihood.ar_loss(net, codes, masks, temperature=0)
    with pytest.raises(TypeError, match="not a model with the PixelCNN's layers"):
        likelihood.ar_loss(object(), codes, masks)
    with pytest.raises(ValueError, match="ar_loss: an ARPlan or the three masks"):
        likelihood.ar_loss(net, codes, masks[:2])
