"""CPU-only: the host side of the decoder's thin layers in training mode (csrc/thin_train.hip, networks/thin_train.py): the C ABI of
libpixelsynth_thin_train.so against its header and bindings, the switch, the sizes the Functions take, the split of the pixels into parts
against its restatement in tests/_thin_train_ref.py, the refusals before anything is launched, and the torch route a block takes on the
host under the opt-in.  Every test here fails on the parent commit, where the module does not exist."""
import os
import re
import types

import pytest
import torch

import _thin_train_ref as ref
from abi_util import ROOT, assert_library_matches_header
from pixelsynth_amd import _lib, _libraries, synthetic as syn
from pixelsynth_amd.networks import architectures as A, conv_routes as C, thin_train as TT
from pixelsynth_amd.networks.routing import Switch


def test_the_registry_has_the_thin_train_library():
    entry = next(e for e in _libraries.LIBRARIES if e.name == "thin_train")
    assert entry.so == "libpixelsynth_thin_train.so" and entry.headers == ("pixelsynth_thin_train.h",)
    assert entry.last_error == "ps_thin_train_last_error"
    assert [u for u, _ in entry.units] == ["thin_train.hip"] and entry.units[0][1] == _libraries.NO_CONTRACT
    protos = assert_library_matches_header("thin_train")
    assert set(protos) == set(_lib.THIN_TRAIN_PROTOS) == {
        "ps_thin_train_last_error", "ps_thin_train_parts", "ps_thin_train_workspace_bytes", "ps_thin_expand_f32", "ps_thin_grad_weight_f32",
        "ps_thin_add_bias_f32"}
    assert _lib.PROTOS["thin_train"] is _lib.THIN_TRAIN_PROTOS and [e.name for e in _libraries.LIBRARIES] == list(_lib.PROTOS)
    header = open(os.path.join(ROOT, "include", "pixelsynth_thin_train.h")).read()
    for name, value in (("MAX_PARTS", ref.MAX_PARTS), ("MIN_PART", ref.MIN_PART), ("GROUPS", ref.GROUPS), ("MAX_WIDE", ref.MAX_WIDE)):
        assert int(re.search(r"#define PS_THIN_TRAIN_%s (\d+)" % name, header).group(1)) == value
    assert TT.MAX_WIDE == ref.MAX_WIDE
    # the pinned library does not export what this one adds
    assert not any(hasattr(_lib.lib(), fn) for fn in protos)
    assert len(_lib.exported_symbols()) == len(_lib._PROTOS) and not any("thin_train" in s or "thin_expand" in s for s in _lib.exported_symbols())


def test_the_switch_resolves_in_the_documented_order_and_defaults_to_torch(monkeypatch):
    sw = TT.decoder_thin_train
    assert isinstance(sw, Switch) and A.decoder_thin_train is sw and sw.name == "decoder_thin_train" and set(sw.values) == {"hip", "torch"}
    assert sw.from_env({}) == "torch" and sw.from_env({"PS_DECODER_THIN_TRAIN": "hip"}) == "hip"
    assert TT.DECODER_THIN_TRAIN == os.environ.get("PS_DECODER_THIN_TRAIN", "torch")
    monkeypatch.setattr(TT, "DECODER_THIN_TRAIN", "torch")
    hip, torch_ = types.SimpleNamespace(decoder_thin_train="hip"), types.SimpleNamespace(decoder_thin_train="torch")
    assert TT.mode() == "torch" and TT.mode(types.SimpleNamespace()) == "torch" and TT.mode(syn.network_opts()) == "torch"
    assert TT.mode(hip) == "hip"                                   # the options over the process default
    monkeypatch.setattr(TT, "DECODER_THIN_TRAIN", "hip")           # the process default, read at every call
    assert TT.mode() == "hip" and TT.mode(torch_) == "torch"
    with sw("torch"):                                              # the block over both
        assert TT.mode() == "torch" and TT.mode(hip) == "torch"
        with sw("hip"):
            assert TT.mode(torch_) == "hip"
        assert TT.mode(hip) == "torch"
    assert sw.forced() is None
    with pytest.raises(ValueError, match="decoder_thin_train: 'hip' or 'torch'"):
        sw("fast")
    monkeypatch.setattr(TT, "DECODER_THIN_TRAIN", "fast")
    with pytest.raises(ValueError, match="PS_DECODER_THIN_TRAIN"):
        TT.mode()


def test_the_sizes_the_functions_take():
    """The decoder's four layers at 256 x 256, and each neighbouring size refused"""
    for kind, Ci, Co, k in ref.DECODER_LAYERS:
        takes, other = (TT.takes_in, TT.takes_out) if kind == "in" else (TT.takes_out, TT.takes_in)
        assert takes(Ci, Co, k, 256, 256) and not other(Ci, Co, k, 256, 256), (kind, Ci, Co, k)
        wstep = 64 if kind == "in" else 32
        for H, W in ((256, 256 + wstep), (8, wstep), (264, 256)):
            assert takes(Ci, Co, k, H, W), (kind, H, W)
        for H, W in ((252, 256), (260, 256), (256, 256 - wstep // 2), (256, 256 + wstep // 2), (0, 256), (256, 0), (257, 256), (256, 257)):
            assert not takes(Ci, Co, k, H, W), (kind, H, W)
        for kk in (0, 2, 5):
            assert not takes(Ci, Co, kk, 256, 256)
    assert TT.takes_in(4, 32, 3, 8, 64) and TT.takes_in(4, 256, 3, 8, 64) and TT.takes_in(4, 96, 3, 8, 64)
    for Ci, Co in ((3, 64), (5, 64), (8, 64), (4, 48), (4, 16), (4, 0), (4, 288), (4, 4)):
        assert not TT.takes_in(Ci, Co, 3, 256, 256) and not TT.takes_in(Ci, Co, 1, 256, 256), (Ci, Co)
    assert not TT.takes_in(4, 96, 1, 256, 256)                        # (the 1 x 1 kernel's own limit on the way back: 96 input channels)
    for T in (1, 2, 3, 4):
        assert TT.takes_out(128, T, 3, 256, 256) and TT.takes_out(32, T, 1, 8, 32) and TT.takes_out(256, T, 3, 8, 32)
    for Ci, Co in ((128, 0), (128, 5), (128, 8), (112, 3), (144, 3), (16, 3), (0, 3), (288, 3)):
        assert not TT.takes_out(Ci, Co, 3, 256, 256) and not TT.takes_out(Ci, Co, 1, 256, 256), (Ci, Co)
    assert TT.takes_out(96, 3, 3, 256, 256) and not TT.takes_out(96, 3, 1, 256, 256)
    # the Functions refuse what they do not take with a ValueError (the caller goes through torch)
    with pytest.raises(ValueError, match="conv_thin_in_train: x must be"):
        TT.conv_thin_in_train(torch.zeros(1, 4, 8, 64), torch.zeros(64, 4, 3, 3))
    with pytest.raises(ValueError, match="conv_thin_out_train: x must be"):
        TT.conv_thin_out_train(torch.zeros(1, 128, 8, 32), torch.zeros(3, 128, 3, 3))


SIZES = [f + (w, T, k) for f in ref.FRAMES + [ref.RAGGED] for w, T, k in ((32, 1, 1), (128, 3, 3), (64, 4, 3))] + [
    (16, 256, 256, 64, 4, 3), (16, 256, 256, 128, 3, 1), (1, 256, 256, 128, 3, 3), (1, 1, 1, 32, 1, 1), (1, 3, 11, 256, 2, 3), (7, 33, 65, 32, 4, 3),
    (128, 256, 256, 64, 4, 3)]


def test_the_part_restatement_covers_every_pixel_once_in_order():
    L = _lib.library("thin_train")
    for B, H, W, Cw, T, k in SIZES:
        npix = B * H * W
        parts = ref.part_ranges(npix)
        assert ref.sizes_ok(B, H, W, Cw, T, k) and len(parts) == L.ps_thin_train_parts(B, H, W, Cw, T, k) and 1 <= len(parts) <= ref.MAX_PARTS
        assert parts[0][0] == 0 and parts[-1][1] == npix and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
        length = parts[0][1] - parts[0][0]
        assert all(hi - lo == length for lo, hi in parts[:-1]) and 0 < parts[-1][1] - parts[-1][0] <= length
        assert len(parts) == 1 or (length >= ref.MIN_PART and length % ref.GROUPS == 0)
        assert L.ps_thin_train_workspace_bytes(B, H, W, Cw, T, k) == ref.workspace_bytes(B, H, W, Cw, T, k)
        for lo, hi in (parts[0], parts[-1]):
            groups = ref.group_pixels(lo, hi)
            assert len(groups) == ref.GROUPS and sorted(p for q in groups for p in q) == list(range(lo, hi)) and all(q == sorted(q) for q in groups)
        assert ref.chain(npix) == -(-length // ref.GROUPS) + ref.GROUPS
    # the shapes the GPU test uses: the ragged one has more than one part and a shorter last one, the largest of the others too has three
    ragged = ref.part_ranges(ref.RAGGED[0] * ref.RAGGED[1] * ref.RAGGED[2])
    assert ragged == [(0, 1024), (1024, 2048), (2048, 2560)]
    assert [len(ref.part_ranges(B * H * W)) for B, H, W in ref.FRAMES] == [1, 2, 3]
    assert len(ref.part_ranges(16 * 256 * 256)) == ref.MAX_PARTS and ref.chain(16 * 256 * 256) == 128 + ref.GROUPS
    assert len(ref.part_ranges(128 * 256 * 256)) == ref.MAX_PARTS
    for bad in ((0, 8, 64, 32, 3, 3), (1, 0, 64, 32, 3, 3), (1, 8, 0, 32, 3, 3), (1, 8, 64, 0, 3, 3), (1, 8, 64, 48, 3, 3), (1, 8, 64, 288, 3, 3),
                (1, 8, 64, 32, 0, 3), (1, 8, 64, 32, 5, 3), (1, 8, 64, 32, 3, 2), (1, 8, 64, 32, 3, 5), (32768, 256, 256, 32, 3, 3), (-1, 8, 64, 32, 3, 3)):
        assert L.ps_thin_train_parts(*bad) == 0 and L.ps_thin_train_workspace_bytes(*bad) == 0 and not ref.sizes_ok(*bad), bad


def test_entry_points_refuse_before_anything_is_launched():
    L = _lib.library("thin_train")
    err = L.ps_thin_train_last_error
    p = torch.zeros(64).data_ptr()                     # (any aligned non-null address: the arguments are refused before it is looked at)
    assert p % 16 == 0
    ok = (1, 8, 64, 32, 3, 3)
    need = L.ps_thin_train_workspace_bytes(*ok)
    names = ("thin", "wide", "B", "H", "W", "Cw", "T", "k", "wide_is_g", "gw", "gb", "ws", "bytes")
    gw = lambda **kw: L.ps_thin_grad_weight_f32(*[kw.get(n, v) for n, v in zip(names, (p, p) + ok + (1, p, p, p, need))], None)  # noqa: E731
    for name in ("thin", "wide", "gw"):
        assert gw(**{name: None}) != 0 and b"null pointer" in err()
    for name in ("wide", "gw"):
        assert gw(**{name: p + 4}) != 0 and b"aligned to 16 bytes" in err()
    assert gw(thin=p + 2) != 0 and gw(gb=p + 2) != 0 and gw(thin=p + 4, T=4) != 0 and b"aligned to 16 bytes" in err()
    for kw in (dict(B=0), dict(Cw=48), dict(Cw=288), dict(T=0), dict(T=5), dict(k=2), dict(H=-8)):
        assert gw(**kw) != 0 and b"Cw a multiple of 32" in err(), kw
    assert gw(wide_is_g=2) != 0 and b"wide_is_g" in err()
    assert gw(ws=None) != 0 and b"null pointer (workspace)" in err()
    assert gw(bytes=need - 1) != 0 and b"workspace of" in err() and str(need).encode() in err()
    assert gw(ws=p + 4) != 0 and b"workspace must be aligned" in err()
    ex = lambda **kw: L.ps_thin_expand_f32(*[kw.get(n, v) for n, v in zip(  # noqa: E731
        ("g", "w", "B", "H", "W", "T", "Cw", "k", "out"), (p, p, 1, 8, 64, 3, 32, 3, p))], None)
    for name in ("g", "w", "out"):
        assert ex(**{name: None}) != 0 and b"null pointer" in err()
    assert ex(w=p + 4) != 0 and ex(out=p + 8) != 0 and ex(g=p + 4, T=4) != 0 and b"aligned to 16 bytes" in err()
    for kw in (dict(W=66), dict(Cw=16), dict(T=5), dict(k=4), dict(B=0)):
        assert ex(**kw) != 0 and b"W a multiple of 4" in err(), kw
    assert L.ps_thin_add_bias_f32(None, p, 8, 3, None) != 0 and b"null pointer" in err()
    assert L.ps_thin_add_bias_f32(p, p, 0, 3, None) != 0 and L.ps_thin_add_bias_f32(p, p, 8, 0, None) != 0 and b"npix and C" in err()
    # through the binding: a CPU tensor is refused by name before a stream is looked up
    with pytest.raises(RuntimeError, match=r"ps_thin_expand_f32: args\[0\] is a CPU tensor.*no CPU fallback"):
        _lib.call("ps_thin_expand_f32", torch.zeros(1, 8, 64, 3), torch.zeros(9, 3, 32), 1, 8, 64, 3, 32, 3, torch.zeros(1, 8, 64, 32))


def test_the_fp64_formulas():
    """gradcheck of the formula the reference differentiates, the header's sums against it, and the bounds: they hold torch's own fp32 and
    not a dropped pixel"""
    gen = torch.Generator().manual_seed(5)
    x, w, b = (torch.randn(s, dtype=torch.float64, generator=gen).requires_grad_() for s in ((1, 2, 3, 4), (3, 2, 3, 3), (3,)))
    assert torch.autograd.gradcheck(lambda *t: torch.nn.functional.conv2d(*t, padding=1), [x, w, b])
    g = torch.randn(1, 3, 3, 4, dtype=torch.float64, generator=gen)
    gx, gw, gb = ref.conv_grads(x, w, b, g)
    H, W = 3, 4
    want_w, want_x = torch.zeros_like(gw), torch.zeros_like(gx)
    for ky in range(3):
        for kx in range(3):
            for y in range(H):
                for xx in range(W):
                    yy, xs = y + ky - 1, xx + kx - 1
                    if 0 <= yy < H and 0 <= xs < W:      # grad_weight[t][j][c] = sum_p g[p][j] x[p + off(t)][c];  grad_input: w[t][j][c] = W[j][c][8 - t]
                        want_w[:, :, ky, kx] += g[0, :, y, xx].view(3, 1) * x.detach()[0, :, yy, xs].view(1, 2)
                        want_x[0, :, y, xx] += (w.detach()[:, :, 2 - ky, 2 - kx] * g[0, :, yy, xs].view(3, 1)).sum(0)
    assert torch.allclose(gw, want_w, rtol=1e-13, atol=1e-13) and torch.allclose(gx, want_x, rtol=1e-13, atol=1e-13)
    assert torch.allclose(gb, g.sum((0, 2, 3)), rtol=1e-13, atol=1e-13)
    assert torch.equal(ref.expand_terms((1, 2, 3, 4), 3, 3)[0, 0], 3 * torch.tensor([[4., 6, 6, 4], [6, 9, 9, 6], [4, 6, 6, 4]], dtype=torch.float64))
    assert torch.equal(ref.expand_terms((1, 2, 3, 4), 2, 1)[0, 0], torch.full((3, 4), 2.0, dtype=torch.float64))
    x, w, b, g = ref.inputs("out", ref.RAGGED, 32, 3, 3)
    g64, g32 = ref.conv_grads(x, w, b, g), ref.conv_grads(x, w, b, g, torch.float32)
    bw, bb = ref.sums_bound(x, w, g)
    assert ref.check("fp32 autograd grad_input", g32[0], g64[0], ref.expand_bound(x, w, g)) < 1.0
    assert ref.check("fp32 autograd grad_weight", g32[1], g64[1], bw) < 1.0 and ref.check("fp32 autograd grad_bias", g32[2], g64[2], bb) < 1.0
    g[0, :, 0, 0] = 0
    dropped = ref.conv_grads(x, w, b, g, torch.float32)
    assert ref.check("grad_weight without a pixel", dropped[1], g64[1], bw) > 1.0 and ref.check("grad_bias without a pixel", dropped[2], g64[2], bb) > 1.0


@pytest.mark.parametrize("ends", [(4, 64), (128, 3)], ids=lambda e: "%dto%d" % e)
def test_on_the_host_a_block_under_the_opt_in_runs_the_torch_route(ends, monkeypatch):
    """A thin block on the CPU under decoder_thin_train("hip") with the other opt-ins on: the same bits as without, the new Functions are
    not entered and no entry point is called"""
    from pixelsynth_amd.networks import block_train as BT, f16x3
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])

    def refuse(*a, **k):
        raise AssertionError("a thin Function on the host")
    monkeypatch.setattr(TT._ConvThinInTrain, "apply", refuse)
    monkeypatch.setattr(TT._ConvThinOutTrain, "apply", refuse)
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(2, ends[0], 8, 64, generator=gen)
    noise = [torch.randn(2, A.NOISE_SZ, generator=gen) for _ in range(2)]
    out = []
    for m in ("torch", "hip"):
        torch.manual_seed(0)
        blk = A.ResNet_Block(ends[0], ends[1], syn.network_opts()).train()
        xg = x.clone().requires_grad_()
        with TT.decoder_thin_train(m), BT.decoder_block_train("hip"), f16x3.decoder_conv_train("f16x3"):
            assert C._thin_train_conv(blk.ch_a[2], xg, blk.opt) is None and C._thin_train_conv(blk.ch_b[0], xg, blk.opt) is None
            y = blk(xg, noise)
        y.square().sum().backward()
        out.append((y.detach(), xg.grad, blk.ch_a[2].weight_orig.grad, blk.ch_b[0].weight_orig.grad, blk.ch_b[0].bias.grad))
    assert all(torch.equal(a, b) for a, b in zip(*out)) and not calls
