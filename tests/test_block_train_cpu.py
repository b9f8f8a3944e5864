"""CPU-only: the host side of a decoder block's training passes (csrc/block_train.hip, networks/block_train.py): the C ABI of
libpixelsynth_block_train.so against its header and bindings, the split of the pixels into parts against its pure-Python mirror, the
refusals before anything is launched, the fp64 formulas of tests/_block_train_ref.py (gradcheck, the adjoint identity); the switch is in
tests/test_decoder_routing_cpu.py."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _block_train_ref as ref
from abi_util import ROOT, assert_library_matches_header
from pixelsynth_amd import _lib, _libraries
from pixelsynth_amd.networks import architectures as A, block_train as BT


def test_the_registry_has_the_block_train_library():
    """Fails on the parent commit: there is no such library"""
    entry = next(e for e in _libraries.LIBRARIES if e.name == "block_train")
    assert entry.so == "libpixelsynth_block_train.so" and entry.headers == ("pixelsynth_block_train.h",)
    assert entry.last_error == "ps_block_train_last_error"
    assert [u for u, _ in entry.units] == ["block_train.hip"] and entry.units[0][1] == _libraries.NO_CONTRACT
    protos = assert_library_matches_header("block_train")
    assert set(protos) == set(_lib.BLOCK_TRAIN_PROTOS) == {
        "ps_block_train_last_error", "ps_conv1x1_grad_weight_parts", "ps_conv1x1_grad_weight_workspace_bytes",
        "ps_conv1x1_grad_weight_f32", "ps_upsample_add_bwd_nhwc_f32", "ps_pool_add_bwd_nhwc_f32"}
    assert _lib.PROTOS["block_train"] is _lib.BLOCK_TRAIN_PROTOS
    header = open(os.path.join(ROOT, "include", "pixelsynth_block_train.h")).read()
    for name, value in (("MAX_PARTS", ref.MAX_PARTS), ("MIN_PART", ref.MIN_PART), ("WAVES", ref.WAVES), ("MAX_CHANNELS", ref.MAX_CHANNELS)):
        assert int(re.search(r"#define PS_BLOCK_TRAIN_%s (\d+)" % name, header).group(1)) == value
    assert BT.MAX_CHANNELS == ref.MAX_CHANNELS
    # the pinned library does not export what this one adds
    assert not any(hasattr(_lib.lib(), fn) for fn in protos)
    assert len(_lib.exported_symbols()) == len(_lib._PROTOS) and not any("block_train" in s or "grad_weight" in s for s in _lib.exported_symbols())


SIZES = ref.GW_SHAPES + [(512, 16, 16), (528, 64, 64), (16 * 256 * 256, 64, 128), (16 * 128 * 128, 128, 256), (16 * 64 * 64, 256, 128),
                         (16 * 128 * 128, 128, 128), (16 * 256 * 256, 256, 256), (16 * 256 * 256 + 16, 64, 64), (2 ** 26, 192, 48), (4096, 80, 208)]


def test_the_part_mirror_covers_every_pixel_once_in_order():
    L = _lib.library("block_train")
    parts_of, ws = L.ps_conv1x1_grad_weight_parts, L.ps_conv1x1_grad_weight_workspace_bytes
    for npix, Ci, Co in SIZES:
        parts = ref.part_ranges(npix, Ci, Co)
        assert len(parts) == parts_of(npix, Ci, Co) and 1 <= len(parts) <= ref.MAX_PARTS, (npix, Ci, Co)
        assert parts[0][0] == 0 and parts[-1][1] == npix and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
        length = parts[0][1] - parts[0][0]
        assert all(hi - lo == length for lo, hi in parts[:-1]) and 0 < parts[-1][1] - parts[-1][0] <= length
        assert all(lo % 16 == 0 and hi % 16 == 0 for lo, hi in parts) and (length >= ref.MIN_PART or len(parts) == 1)
        least = len(parts) * (Co * Ci + Co) * 4
        assert least <= ws(npix, Ci, Co) < least + 256 and ws(npix, Ci, Co) % 256 == 0
        TO, TC, tiles = ref.tiles(Ci, Co)
        assert TO * TC <= 2 and tiles * TO * TC == -(-Co // 64) * -(-Ci // 64)
        # inside a part: the wavefronts' pixels are the part's, each once, and every group of four stays together
        for lo, hi in (parts[0], parts[-1]):
            if hi - lo > 2 ** 16:
                continue
            waves = ref.wave_pixels(lo, hi)
            assert sorted(p for w in waves for p in w) == list(range(lo, hi)) and all(w == sorted(w) and len(w) % 4 == 0 for w in waves)
        assert ref.chain(npix, Ci, Co) == 4 * -(-(length // 4) // ref.WAVES) + ref.WAVES
    assert len(ref.part_ranges(16, 64, 64)) == 1 and len(ref.part_ranges(512, 256, 128)) == 1
    three = ref.part_ranges(1040, 128, 256)
    assert three == [(0, 512), (512, 1024), (1024, 1040)]                                  # a short last part
    assert len(ref.part_ranges(16 * 256 * 256, 64, 128)) == ref.MAX_PARTS                  # the maximum: work for every compute unit
    assert len(ref.part_ranges(16 * 256 * 256, 256, 256)) == 64                            # eight workgroups per part there
    for bad in ((0, 64, 64), (8, 64, 64), (24, 64, 64), (64, 0, 64), (64, 64, 0), (64, 8, 64), (64, 64, 72), (64, 272, 64), (64, 64, 512),
                (64, -64, 64)):
        assert parts_of(*bad) == 0 and ws(*bad) == 0 and not ref.sizes_ok(*bad) and ref.part_ranges(*bad) == [], bad


def test_entry_points_refuse_before_anything_is_launched():
    L = _lib.library("block_train")
    err = L.ps_block_train_last_error
    p = torch.zeros(64).data_ptr()                     # (any aligned non-null address: the arguments are refused before it is looked at)
    assert p % 16 == 0
    need = L.ps_conv1x1_grad_weight_workspace_bytes(1040, 128, 256)
    gw = lambda **kw: L.ps_conv1x1_grad_weight_f32(*[kw.get(n, v) for n, v in zip(  # noqa: E731
        ("x", "g", "npix", "Ci", "Co", "gw", "gb", "ws", "bytes"), (p, p, 1040, 128, 256, p, p, p, need))], None)
    for name in ("x", "g", "gw"):
        assert gw(**{name: None}) != 0 and b"null pointer" in err()
        assert gw(**{name: p + 4}) != 0 and b"aligned to 16 bytes" in err()
    assert gw(gb=p + 8) != 0 and b"aligned to 16 bytes" in err()
    for kw in (dict(npix=0), dict(npix=1032), dict(Ci=72), dict(Co=0), dict(Co=272), dict(Ci=-16)):
        assert gw(**kw) != 0 and b"multiples of 16" in err(), kw
    assert gw(ws=None) != 0 and b"null pointer (workspace)" in err()
    assert gw(bytes=need - 1) != 0 and b"workspace of" in err() and str(need).encode() in err()
    assert gw(ws=p + 4) != 0 and b"workspace must be aligned" in err()
    for fn, tag, ok in ((L.ps_upsample_add_bwd_nhwc_f32, b"upsample_add_bwd", (1, 1, 3, 4)), (L.ps_pool_add_bwd_nhwc_f32, b"pool_add_bwd", (1, 2, 2, 4))):
        assert fn(None, *ok, p, None) != 0 and b"null pointer" in err() and tag in err()
        assert fn(p, *ok, None, None) != 0 and b"null pointer" in err()
        assert fn(p + 4, *ok, p, None) != 0 and b"aligned to 16 bytes" in err()
        for bad in ((0,) + ok[1:], ok[:3] + (6,), ok[:3] + (0,), (1, 0, 4, 4), (1, 4, 0, 4)):
            assert fn(p, *bad, p, None) != 0 and tag in err(), bad
    assert L.ps_pool_add_bwd_nhwc_f32(p, 1, 3, 4, 4, p, None) != 0 and b"even H, W" in err()
    assert L.ps_pool_add_bwd_nhwc_f32(p, 1, 4, 5, 4, p, None) != 0 and b"even H, W" in err()
    # through the binding: a CPU tensor is refused by name before a stream is looked up
    with pytest.raises(RuntimeError, match=r"ps_pool_add_bwd_nhwc_f32: args\[0\] is a CPU tensor.*no CPU fallback"):
        _lib.call("ps_pool_add_bwd_nhwc_f32", torch.zeros(1, 1, 1, 4), 1, 2, 2, 4, torch.zeros(1, 2, 2, 4))
    # and the Functions refuse what they do not take with a ValueError (the caller goes through torch)
    with pytest.raises(ValueError, match="conv1x1_train: x must be"):
        BT.conv1x1_train(torch.zeros(1, 64, 4, 4), torch.zeros(64, 64, 1, 1))
    with pytest.raises(ValueError, match="resample_sum_train"):
        BT.resample_sum_train("Up", torch.zeros(1, 4, 2, 2), None)


@pytest.mark.parametrize("kind", ["Up", "Down"])
def test_gradcheck_and_the_adjoint_identity_in_fp64(kind):
    gen = torch.Generator().manual_seed(4)
    for B, H, W, C in (ref.UP_SHAPES if kind == "Up" else ref.DOWN_SHAPES):
        shape = (B, min(C, 4), H, W)           # (the channels are independent: four of them say what sixty-four would)
        a = torch.randn(shape, dtype=torch.float64, generator=gen)
        Ra = ref.resample(kind, a)
        assert Ra.shape == (B, shape[1], 2 * H, 2 * W) if kind == "Up" else Ra.shape == (B, shape[1], H // 2, W // 2)
        g = torch.randn(Ra.shape, dtype=torch.float64, generator=gen)
        Rtg = ref.adjoint(kind, g, shape)
        lhs, rhs = (Ra * g).sum().item(), (a * Rtg).sum().item()
        assert abs(lhs - rhs) <= 1e-12 * (Ra.abs() * g.abs()).sum().item(), (kind, shape)
        if H * W <= 8:
            assert torch.autograd.gradcheck(lambda t: ref.resample(kind, t), [a.clone().requires_grad_()])
        # the weights a pixel hears with add up to the outputs per input: 4 for "Up"; for "Down" 1/9 per output, 1, 2 or 4 of them
        total = ref.adjoint(kind, torch.ones_like(g), shape)
        terms = ref.adjoint_terms(kind, shape)
        if kind == "Up":
            assert abs(total.sum().item() - 4 * a.numel()) < 1e-9 and terms.max() <= 16 and terms.min() >= (1 if H == 1 or W == 1 else 4)
        else:
            assert set((total * 9).round().flatten().tolist()) <= {1.0, 2.0, 4.0} and torch.equal((total * 9).round() + 1, terms)
            assert (total * 9).round()[0, 0, 1, 1].item() == (1.0 if (H, W) == (2, 2) else 4.0)           # an odd pixel whose second output is out of range


def test_gradcheck_of_the_conv1x1_formula():
    gen = torch.Generator().manual_seed(5)
    x, w, b = (torch.randn(s, dtype=torch.float64, generator=gen).requires_grad_() for s in ((2, 3, 2, 2), (4, 3, 1, 1), (4,)))
    assert torch.autograd.gradcheck(lambda *t: F.conv2d(*t), [x, w, b])
    g = torch.randn(2, 4, 2, 2, dtype=torch.float64, generator=gen)
    gx, gw, gb = ref.conv1x1_grads(x, w, b, g)
    # the header's formulas
    g2, x2 = g.permute(1, 0, 2, 3).reshape(4, -1), x.detach().permute(1, 0, 2, 3).reshape(3, -1)
    assert torch.allclose(gw.view(4, 3), g2 @ x2.t(), rtol=1e-13, atol=1e-13) and torch.allclose(gb, g2.sum(1), rtol=1e-13, atol=1e-13)
    assert torch.allclose(gx, torch.einsum("bohw,oc->bchw", g, w.detach().view(4, 3)), rtol=1e-13, atol=1e-13)
    # the grad_weight bound holds torch's own fp32 and not a dropped pixel
    npix, Ci, Co = ref.GW_SHAPES[1]
    x, w, b, g = ref.gw_inputs(npix, Ci, Co)
    w64 = ref.conv1x1_grads(x, w, b, g)[1]
    w32 = ref.conv1x1_grads(x, w, b, g, torch.float32)[1]
    bound = ref.grad_weight_bound(x, g, npix, Ci, Co)
    assert ref.check("fp32 autograd grad_weight", w32, w64, bound) < 1.0
    g[0, :, 0, 0] = 0
    assert ref.check("grad_weight without a pixel", ref.conv1x1_grads(x, w, b, g, torch.float32)[1], w64, bound) > 1.0


def test_on_the_host_the_opt_in_changes_nothing(monkeypatch):
    """A block on the CPU under decoder_block_train("hip"): the same bits as without, and no entry point is called"""
    from pixelsynth_amd import synthetic as syn
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(2, 64, 4, 4, generator=gen)
    noise = [torch.randn(2, A.NOISE_SZ, generator=gen) for _ in range(2)]
    out = []
    for m in ("torch", "hip"):
        torch.manual_seed(0)
        blk = A.ResNet_Block(64, 64, syn.network_opts(), "Down").train()
        xg = x.clone().requires_grad_()
        with BT.decoder_block_train(m):
            y = blk(xg, noise)
        y.square().sum().backward()
        out.append((y.detach(), xg.grad, blk.ch_b[0].weight_orig.grad))
    assert all(torch.equal(a, b) for a, b in zip(*out)) and not calls
