"""CPU-only: the host side of the split-fp16 convolution's backward pass (csrc/conv_bwd.hip, networks/f16x3.py): the library against its
header and bindings, the helper's fp64 formulas against fp64 autograd of F.conv2d at three gradient scales, the scale rule at its edges,
the mirror of the split into parts against the library, and the opt-in's default."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _conv_bwd_ref as ref
from abi_util import ROOT, assert_library_matches_header
from pixelsynth_amd import _lib, _libraries
from pixelsynth_amd.networks import architectures as A, f16x3


def test_the_registry_has_the_conv_bwd_library():
    entry = next(e for e in _libraries.LIBRARIES if e.name == "conv_bwd")
    assert entry.so == "libpixelsynth_conv_bwd.so" and entry.headers == ("pixelsynth_conv_bwd.h",)
    assert entry.last_error == "ps_conv_bwd_last_error"
    assert [u for u, _ in entry.units] == ["conv_bwd.hip"] and entry.units[0][1] == _libraries.NO_CONTRACT
    protos = assert_library_matches_header("conv_bwd")
    assert set(protos) == set(_lib.CONV_BWD_PROTOS) == {
        "ps_conv_bwd_last_error", "ps_conv3x3_bwd_workspace_bytes", "ps_conv3x3_bwd_parts", "ps_conv3x3_bwd_prepare_f32",
        "ps_conv3x3_grad_weight_f16x3", "ps_conv3x3_bwd_unscale_f32"}
    header = open(os.path.join(ROOT, "include", "pixelsynth_conv_bwd.h")).read()
    assert int(re.search(r"#define PS_CONV_BWD_MAX_PARTS (\d+)", header).group(1)) == ref.MAX_PARTS
    # the pinned library does not export what this one adds
    assert not any(hasattr(_lib.lib(), fn) for fn in protos)


def test_the_formula_is_as_good_as_fp32_once_the_gradient_is_scaled():
    """T against fp64 autograd of F.conv2d on B = 2, 32 x 32, 32 -> 64 at gradient scales 1, 1e-4, 1e-7: the scaled split stays at the
    1e-7 (weight) / 3e-7 (input) of max |ref| it has at scale 1 -- one and a half times the largest figure measured with it is the bound
    -- and sits well inside torch's own fp32 error; the UNSCALED split (s forced to 1) loses the small gradients."""
    gen = torch.Generator().manual_seed(5)
    x = torch.relu(torch.randn(2, 32, 32, 32, generator=gen) * 1.5)
    w = torch.randn(64, 32, 3, 3, generator=gen) / (3 * 32 ** 0.5)
    g0 = torch.randn(2, 64, 32, 32, generator=gen)
    for scale in (1.0, 1e-4, 1e-7):
        g = g0 * scale
        r = ref.reference(x, w, g)
        # the helper's unsplit gradients are fp64 autograd's
        xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
        ax, aw = torch.autograd.grad(F.conv2d(xd, wd, None, 1, 1), (xd, wd), g.double())
        assert torch.allclose(r.x.g64, ax, rtol=0, atol=1e-12 * ax.abs().max().item())
        assert torch.allclose(r.weight.g64, aw, rtol=0, atol=1e-12 * aw.abs().max().item())
        ew = (r.weight.T - aw).abs().max().item() / aw.abs().max().item()
        ex = (r.x.T - ax).abs().max().item() / ax.abs().max().item()
        e32 = r.weight.E32 / aw.abs().max().item()
        print(f"scale {scale:g}: s = 2^{int(math.log2(r.s))}, T error / max |ref| weight {ew:.2e} input {ex:.2e}; torch fp32 weight {e32:.2e}")
        assert ew <= 1.5 * 8.5e-8 and ex <= 1.5 * 3.0e-7, (scale, ew, ex)
        assert ew <= 0.5 * e32, (scale, ew, e32)
        assert 2 ** 14 <= (g * r.s).abs().max().item() < 2 ** 15
    # without the scaling: the split of g = 1e-7 * randn keeps 2^-25 absolute
    gh, gl = ref.split(g)
    xh, xl = ref.split(x)
    d = torch.double
    unscaled = ref.wgrad(xh.to(d) + xl.to(d), gh.to(d)) + ref.wgrad(xh.to(d), gl.to(d))
    assert (unscaled - aw).abs().max().item() / aw.abs().max().item() > 1e-2


def test_the_scale_rule_at_its_edges():
    for m in (0.0, math.inf, math.nan, -0.0):
        assert ref.scale_of(m) == 1.0
    f32 = lambda v: torch.tensor(v, dtype=torch.float64).float().item()
    for k in (-149, -140, -126, -30, -24, -1, 0, 1, 14, 15, 16, 100, 127):
        for m in (f32(2.0 ** k), f32(2.0 ** k * (1 - 2.0 ** -24))):
            if m == 0.0 or k == -149 and m != 2.0 ** -149:
                continue
            s = ref.scale_of(m)
            e = math.frexp(m)[1]
            assert s == 2.0 ** max(-126, min(126, 15 - e)) and math.frexp(s)[0] == 0.5          # a power of two
            assert f32(s) == s and f32(1 / s) == 1 / s and s >= 2.0 ** -126 and 1 / s >= 2.0 ** -126   # s and 1 / s: normal fp32
            if -111 <= e <= 128:                                                                # (the exponent is not held)
                assert 2 ** 14 <= m * s < 2 ** 15, (k, m, s)
            else:
                assert m * s < 2 ** 15
    assert ref.scale_of(1.0) == 2.0 ** 14 and ref.scale_of(f32(1 - 2.0 ** -24)) == 2.0 ** 15
    assert ref.scale_of(3e-8) * 3e-8 >= 2 ** 14


def test_the_parts_cover_every_pixel_tile_once_and_mirror_the_library():
    L = _lib.library("conv_bwd")
    shapes = ref.SHAPES + [(1, 16, 16, 64, 64), (16, 256, 256, 64, 64), (16, 256, 256, 128, 128), (16, 128, 128, 128, 256),
                           (16, 128, 128, 256, 256), (16, 64, 64, 256, 256), (16, 64, 64, 256, 128), (4, 48, 16, 64, 64), (2, 16, 80, 512, 512)]
    for B, H, W, Ci, Co in shapes:
        rs = ref.part_ranges(B, H, W, Ci, Co)
        assert 1 <= len(rs) <= ref.MAX_PARTS
        assert rs[0][0] == 0 and rs[-1][1] == ref.tiles(B, H, W) and all(a[1] == b[0] for a, b in zip(rs, rs[1:]))   # consecutive, complete
        assert all(lo < hi for lo, hi in rs)                                                                              # no empty part
        assert len(rs) == L.ps_conv3x3_bwd_parts(B, H, W, Ci, Co), (B, H, W, Ci, Co)
        ws = L.ps_conv3x3_bwd_workspace_bytes(B, H, W, Ci, Co)
        assert ws >= len(rs) * 9 * Ci * Co * 4 and ws % 256 == 0
    assert len(ref.part_ranges(16, 256, 256, 64, 64)) == 256                       # one workgroup on each of 256 compute units
    assert L.ps_conv3x3_bwd_workspace_bytes(16, 64, 64, 256, 256) <= 100 << 20      # tens of MB
    assert len(ref.part_ranges(1, 16, 16, 64, 64)) == 1
    last = ref.part_ranges(3, 16, 48, 128, 64)
    assert len(last) > 1 and last[-1][1] - last[-1][0] < last[0][1] - last[0][0]    # several parts, the last one partial
    for bad in ((0, 16, 16, 64, 64), (1, 8, 16, 64, 64), (1, 16, 24, 64, 64), (1, 16, 16, 32, 64), (1, 16, 16, 64, 96), (1, 16, 16, 0, 64),
                (1, 2048, 2048, 512, 64), (-1, 16, 16, 64, 64)):
        assert L.ps_conv3x3_bwd_workspace_bytes(*bad) == 0 and L.ps_conv3x3_bwd_parts(*bad) == 0, bad


def test_entry_points_refuse_before_anything_is_launched():
    L = _lib.library("conv_bwd")
    p = torch.zeros(64).data_ptr() // 16 * 16 + 16
    B, H, W, Ci, Co = 1, 16, 16, 64, 64
    need = L.ps_conv3x3_bwd_workspace_bytes(B, H, W, Ci, Co)
    err = lambda: L.ps_conv_bwd_last_error().decode()
    assert L.ps_conv3x3_bwd_prepare_f32(None, B, H, W, Co, p, p, None, p, need, None) < 0 and "null" in err()
    assert L.ps_conv3x3_bwd_prepare_f32(p, B, H, W, Co, p, p, None, p, need, None) < 0 and "cannot be g" in err()
    assert L.ps_conv3x3_bwd_prepare_f32(p, B, H, 24, Co, p + 16, p, None, p, need, None) < 0 and "multiples of 16" in err()
    assert L.ps_conv3x3_bwd_prepare_f32(p, B, H, W, Co, p + 16, p, None, p, 16, None) < 0 and "workspace" in err()
    assert L.ps_conv3x3_grad_weight_f16x3(p, p, p, B, H, W, Ci, Co, p, None, p, need, None) < 0 and "null" in err()
    assert L.ps_conv3x3_grad_weight_f16x3(p, p, p, B, H, W, 32, Co, p, p, p, need, None) < 0 and "multiples of 64" in err()
    assert L.ps_conv3x3_grad_weight_f16x3(p, p, p, B, H, W, Ci, Co, p, p, p, need - 1, None) < 0 and "workspace" in err()
    assert L.ps_conv3x3_grad_weight_f16x3(p + 4, p, p, B, H, W, Ci, Co, p, p, p, need, None) < 0 and "aligned" in err()
    assert L.ps_conv3x3_bwd_unscale_f32(p, 6, p, None) < 0 and "multiple of 4" in err()
    assert L.ps_conv3x3_bwd_unscale_f32(None, 8, p, None) < 0 and "null" in err()


def test_the_opt_in_defaults_to_fp32(monkeypatch):
    """(the switch itself: tests/test_decoder_routing_cpu.py)"""
    assert f16x3.decoder_conv_train.from_env({}) == "fp32"
    assert f16x3.DECODER_CONV_TRAIN == os.environ.get("PS_DECODER_CONV_TRAIN", "fp32")
    monkeypatch.setattr(f16x3, "DECODER_CONV_TRAIN", "fp32")
    assert f16x3.train_mode() == "fp32"
    # on the host nothing is taken: a CPU convolution in grad mode under the opt-in stays torch's
    conv = torch.nn.Conv2d(64, 64, 3, 1, 1)
    x = torch.randn(1, 64, 16, 16, requires_grad=True)
    with f16x3.decoder_conv_train("f16x3"):
        assert A._f16x3_train_conv(conv, x) is None
        y, b = A._conv_split(conv, x)
    assert b is None and torch.equal(y, conv(x))
    with pytest.raises(ValueError):
        f16x3.conv3x3_train(x, conv.weight, conv.bias)
    assert f16x3.train_takes(64, 128, 16, 48) and not f16x3.train_takes(32, 64, 16, 16) and not f16x3.train_takes(64, 64, 16, 24)
