"""CPU-only: the host side of the training-mode batch norm (csrc/norm_train.hip, networks/norm_train.py, the blocks of
networks/architectures.py in train()): the C ABI of libpixelsynth_norm_train.so against its header and bindings, the split into parts,
its refusals before anything is launched, the fp64 formulas of tests/_norm_train_ref.py against torch autograd, a decoder block in
train() on the host -- output, running and standing statistics, reset_stats -- and the route switch."""
import os
import re

import pytest
import torch

import _norm_train_ref as ref
from abi_util import ROOT, assert_library_matches_header
from pixelsynth_amd import _lib, _libraries, synthetic as syn
from pixelsynth_amd.networks import architectures as A, norm_train as NT


def test_the_registry_has_the_norm_train_library():
    entry = next(e for e in _libraries.LIBRARIES if e.name == "norm_train")
    assert entry.so == "libpixelsynth_norm_train.so" and entry.headers == ("pixelsynth_norm_train.h",)
    assert entry.last_error == "ps_norm_train_last_error"
    assert [u for u, _ in entry.units] == ["norm_train.hip"] and entry.units[0][1] == _libraries.NO_CONTRACT
    protos = assert_library_matches_header("norm_train")
    assert set(protos) == set(_lib.NORM_TRAIN_PROTOS) == {
        "ps_norm_train_last_error", "ps_norm_train_workspace_bytes", "ps_norm_train_parts", "ps_norm_train_stats_f32",
        "ps_norm_train_apply_f32", "ps_norm_train_backward_f32"}
    assert _lib.PROTOS["norm_train"] is _lib.NORM_TRAIN_PROTOS
    header = open(os.path.join(ROOT, "include", "pixelsynth_norm_train.h")).read()
    for name, value in (("MAX_PARTS", ref.MAX_PARTS), ("PART_ROWS", ref.PART_ROWS), ("MAX_C", ref.MAX_C)):
        assert int(re.search(r"#define PS_NORM_TRAIN_%s (\d+)" % name, header).group(1)) == value
    # the pinned library does not export what this one adds
    assert not any(hasattr(_lib.lib(), fn) for fn in protos)
    assert len(_lib.exported_symbols()) == len(_lib._PROTOS) and not any("norm_train" in s for s in _lib.exported_symbols())


SIZES = [(1, 1, 4), (1, 512, 4), (1, 513, 8), (3, 240, 4), (2, 3840, 128), (16, 65536, 64), (16, 16384, 256), (1, 512 * 512, 64),
         (1, 512 * 512 + 1, 64), (512, 700, 4), (600, 1025, 4), (7, 100000, 12)]


def test_the_parts_are_consecutive_complete_and_never_empty():
    parts_of = _lib.library("norm_train").ps_norm_train_parts
    ws = _lib.library("norm_train").ps_norm_train_workspace_bytes
    for B, HW, C in SIZES:
        parts = ref.part_ranges(B, HW)
        rows = ref.part_rows(B, HW)
        assert len(parts) == parts_of(B, HW, C), (B, HW, C)
        assert rows % ref.PART_ROWS == 0 and all(r1 > r0 and r1 - r0 <= rows for _, r0, r1 in parts)
        flat = [(b, r) for b, r0, r1 in parts for r in (r0, r1 - 1)]
        assert flat == sorted(flat)
        for b in range(0, B, max(1, B // 3)):
            mine = [(r0, r1) for f, r0, r1 in parts if f == b]
            assert mine[0][0] == 0 and mine[-1][1] == HW and all(a[1] == n[0] for a, n in zip(mine, mine[1:]))
            assert len(mine) <= max(1, ref.MAX_PARTS // B)
            assert rows == ref.PART_ROWS or -(-HW // (rows - ref.PART_ROWS)) > max(1, ref.MAX_PARTS // B)      # (the smallest such multiple)
        # one row of (2, C) doubles per part and per frame, 2 C floats; three aligned regions
        least = len(parts) * 2 * C * 8 + B * 2 * C * 8 + 2 * C * 4
        assert least <= ws(B, HW, C) <= least + 3 * 256 and ws(B, HW, C) % 256 == 0
    assert len(ref.part_ranges(1, 512)) == 1 and len(ref.part_ranges(3, 240)) == 3                           # one part (per frame) only
    two = ref.part_ranges(1, 513)
    assert len(two) == 2 and two[1][2] - two[1][1] == 1                                                       # a partial last part
    assert len(ref.part_ranges(1, 512 * 512)) == ref.MAX_PARTS and len(ref.part_ranges(1, 512 * 512 + 1)) == 257     # the maximum; past it: longer parts
    assert len(ref.part_ranges(16, 65536)) == ref.MAX_PARTS >= 256                                            # work for every compute unit
    for bad in ((0, 16, 4), (-1, 16, 4), (2, 0, 4), (2, -7, 4), (2, 16, 0), (2, 16, 6), (2, 16, -4), (2, 16, ref.MAX_C + 4),
                (1, 2 ** 29, 4), (2 ** 16, 2 ** 15, 4)):
        assert parts_of(*bad) == 0 and ws(*bad) == 0 and not ref.sizes_ok(*bad), bad
    assert parts_of(1, 2 ** 29 - 1, 4) > 0 and ref.sizes_ok(1, 2 ** 29 - 1, 4)


def test_entry_points_refuse_before_anything_is_launched():
    L = _lib.library("norm_train")
    err = L.ps_norm_train_last_error
    p = torch.zeros(64).data_ptr()                     # (any aligned non-null address: the arguments are refused before it is looked at)
    assert p % 16 == 0
    B, HW, C = 2, 700, 8
    need = L.ps_norm_train_workspace_bytes(B, HW, C)
    assert need > 0

    def calls(fn, names, ok):
        def bad(**kw):
            assert set(kw) <= set(names), kw
            return fn(*[kw.get(n, v) for n, v in zip(names, ok)], None)
        return bad

    stats = calls(L.ps_norm_train_stats_f32, ["x", "pend", "B", "HW", "C", "eps", "keep", "momentum", "sm", "sv", "mean", "var", "rstd", "ws", "bytes"],
                  [p, p, B, HW, C, 1e-5, 0.9, 0.1, p, p, p, p, p, p, need])
    apply = calls(L.ps_norm_train_apply_f32, ["x", "mean", "rstd", "gain", "bias", "B", "HW", "C", "relu", "y"], [p, p, p, p, p, B, HW, C, 1, p])
    bwd = calls(L.ps_norm_train_backward_f32, ["x", "dy", "mean", "rstd", "gain", "bias", "B", "HW", "C", "relu", "dx", "dgain", "dbias", "ws", "bytes"],
                [p, p, p, p, p, p, B, HW, C, 1, p, p, p, p, need])
    for name, fn, pointers, optional in (("stats", stats, ("x", "sm", "sv", "mean", "var", "rstd"), "pend"),
                                         ("apply", apply, ("x", "mean", "rstd", "gain", "bias", "y"), None),
                                         ("backward", bwd, ("x", "dy", "mean", "rstd", "gain", "bias", "dgain", "dbias"), "dx")):
        tag = f"norm_train_{name}".encode()
        for ptr_name in pointers:
            assert fn(**{ptr_name: None}) != 0 and b"null pointer" in err() and tag in err(), (name, ptr_name)
            assert fn(**{ptr_name: p + 4}) != 0 and b"aligned to 16 bytes" in err() and tag in err(), (name, ptr_name)
        if optional:
            assert fn(**{optional: p + 8}) != 0 and b"aligned to 16 bytes" in err()
        for size in ("B", "HW", "C"):
            for v in (0, -3):
                assert fn(**{size: v}) != 0 and f"{size} = {v}".encode() in err() and b"expected all >= 1" in err() and tag in err()
        assert fn(C=6) != 0 and b"C = 6 is not a multiple of 4" in err() and tag in err()
        assert fn(C=ref.MAX_C + 4) != 0 and b"more than 65536 channels" in err()
        assert fn(HW=2 ** 29) != 0 and b"a frame of 2^31 elements or more" in err()
        assert fn(B=2 ** 16, HW=2 ** 15) != 0 and b"2^31 rows or more" in err()
        if name != "apply":
            assert fn(ws=None) != 0 and b"null pointer (workspace)" in err()
            assert fn(bytes=0) != 0 and b"workspace of 0 bytes" in err()
            assert fn(bytes=need - 1) != 0 and b"workspace of" in err() and str(need).encode() in err()
            assert fn(ws=p + 4) != 0 and b"workspace must be aligned to 16 bytes" in err()
    # through the binding: a CPU tensor is refused by name before a stream is looked up
    z = torch.zeros(8)
    with pytest.raises(RuntimeError, match=r"ps_norm_train_apply_f32: args\[0\] is a CPU tensor.*no CPU fallback"):
        _lib.call("ps_norm_train_apply_f32", torch.zeros(1, 2, 8), z, z, z, z, 1, 2, 8, 1, torch.zeros(1, 2, 8))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shared", [False, True])
def test_the_fp64_formulas_against_autograd(relu, shared):
    eps = 1e-5
    x, gain, bias, dy = ref.inputs(3, 4, 5, 3, seed=2, shared=shared)
    want = ref.autograd(x, gain, bias, dy, eps, relu, torch.float64)
    dx, dgain, dbias = ref.backward64(x, dy, gain.expand(3, 4), bias.expand(3, 4), eps, relu)
    if shared:          # (one row expanded: its gradient is the sum over the samples)
        dgain, dbias = dgain.sum(0, keepdim=True), dbias.sum(0, keepdim=True)
    for name, got, w in zip(("dx", "dgain", "dbias"), (dx, dgain, dbias), want):
        assert got.shape == w.shape and (got - w).abs().max() <= 1e-12 * w.abs().max(), name
    f = ref.forward64(x, gain.expand(3, 4), bias.expand(3, 4), eps, relu)
    assert (f["y"] - ref.composition(x.double(), gain.double(), bias.double(), eps, relu)).abs().max() <= 1e-13
    # the torch route that ships is that composition: same values, and gradcheck on 2 x 4 x 3 x 3
    layer = A.bn(4)
    y = NT.formula(x.double(), gain.double().view(-1, 4, 1, 1), bias.double().view(-1, 4, 1, 1), layer.train(), relu)
    assert (y - f["y"]).abs().max() <= 1e-13
    xs, gs, bs, _ = ref.inputs(2, 4, 3, 3, seed=5, shared=shared)
    args = [t.double().requires_grad_() for t in (xs, gs, bs)]
    assert torch.autograd.gradcheck(lambda a, b, c: NT.formula(a, b.view(-1, 4, 1, 1), c.view(-1, 4, 1, 1), layer, relu), args)
    assert torch.autograd.gradcheck(lambda a, b, c: NT.batch_norm_train(a, b, c, layer, relu), args)
    # the rule for gradients holds torch's own fp32 and not a dropped term
    g32 = ref.autograd(x, gain, bias, dy, eps, relu, torch.float32)
    bound, E32 = ref.grad_bound(g32[0], want[0])
    assert ref.check("fp32 autograd dx", g32[0], want[0], bound) <= 0.25 + 1e-9
    assert ref.check("dx without the k2 term", (dx + 1e-3 * dx.abs().max()).float(), want[0], bound) > 1.0


def _block_case(seed=3):
    gen = torch.Generator().manual_seed(seed)
    x = 0.3 + 1.5 * torch.randn(3, 8, 6, 5, generator=gen)
    noise = [torch.randn(3, A.NOISE_SZ, generator=gen) for _ in range(2)]
    return x, noise


def _expected_block(blk, x, noise):
    """The block by hand on batch statistics: (norm, ReLU, 3 x 3) twice, the 1 x 1 branch added; -> output, [(mean, var)] per norm"""
    stats, h = [], x
    for layer, conv, n in ((blk.ch_a[0], blk.ch_a[2], noise[0]), (blk.ch_a[3], blk.ch_a[5], noise[1])):
        gain, bias = 1 + layer.gain(n), layer.bias(n)
        m, var, _ = (t.to(h.dtype) for t in ref.stats64(h))
        stats.append((m, var))
        h = conv(ref.composition(h, gain, bias, layer.bn.eps, True))
    return h + blk.ch_b[0](x), stats


def test_a_decoder_block_trains_on_the_host():
    """Fails on the parent commit: bn.scale_shift raised in training mode"""
    torch.manual_seed(0)
    blk = A.ResNet_Block(8, 16, syn.network_opts()).train()
    x, noise = _block_case()
    xg = x.clone().requires_grad_()
    y = blk(xg, noise)
    y.square().sum().backward()
    assert y.shape == (3, 16, 6, 5) and xg.grad is not None and torch.isfinite(xg.grad).all() and xg.grad.abs().max() > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in blk.parameters())
    # the first norm's statistics are those of x, whatever the (spectral-normalised) weights; the second's have moved
    m, var, _ = (t.float() for t in ref.stats64(x))
    first, second = blk.ch_a[0].bn, blk.ch_a[3].bn
    assert torch.allclose(first.stored_mean, m * first.momentum, rtol=1e-5, atol=1e-7)
    assert torch.allclose(first.stored_var, 1 - first.momentum + var * first.momentum, rtol=1e-5, atol=1e-7)
    assert second.stored_mean.abs().min() > 0 and (second.stored_var - 1).abs().min() > 0
    assert first.accumulation_counter.item() == 0 and second.accumulation_counter.item() == 0


def test_block_output_is_the_formula_on_batch_statistics():
    """Plain (not spectral) layers, so that the hand-written block has the block's weights exactly"""
    torch.manual_seed(1)
    blk = A.ResNet_Block(8, 16, syn.network_opts(norm_G="sync:batch")).train()
    x, noise = _block_case(4)
    with torch.no_grad():
        want, stats = _expected_block(blk, x, noise)
    y = blk(x.clone().requires_grad_(), noise)
    assert y.requires_grad and (y.detach() - want).abs().max() <= 1e-5 * want.abs().max()
    for layer, (m, var) in zip((blk.ch_a[0], blk.ch_a[3]), stats):
        mom = layer.bn.momentum
        assert torch.allclose(layer.bn.stored_mean, m * mom, rtol=1e-5, atol=1e-6)
        assert torch.allclose(layer.bn.stored_var, 1 - mom + var * mom, rtol=1e-5, atol=1e-6)
    # a second pass moves them again by the momentum rule
    before = [(l.bn.stored_mean.clone(), l.bn.stored_var.clone()) for l in (blk.ch_a[0], blk.ch_a[3])]
    with torch.no_grad():
        y2 = blk(x, noise)
    assert (y2 - want).abs().max() <= 1e-5 * want.abs().max()
    for layer, (m, var), (m0, v0) in zip((blk.ch_a[0], blk.ch_a[3]), stats, before):
        assert torch.allclose(layer.bn.stored_mean, m0 * 0.9 + m * 0.1, rtol=1e-5, atol=1e-6)
        assert torch.allclose(layer.bn.stored_var, v0 * 0.9 + var * 0.1, rtol=1e-5, atol=1e-6)


def test_standing_statistics_add_count_reset_and_serve_eval():
    torch.manual_seed(2)
    blk = A.ResNet_Block(8, 16, syn.network_opts(norm_G="sync:batch")).train()
    norms = [m for m in blk.modules() if isinstance(m, A.bn)]
    assert len(norms) == 2
    for m in norms:
        m.accumulate_standing = True
        m.stored_mean.fill_(3.0)
        m.accumulation_counter.fill_(7.0)
        m.reset_stats()
        assert not m.stored_mean.any() and not m.stored_var.any() and m.accumulation_counter.item() == 0
    cases = [_block_case(s) for s in (5, 6, 7)]
    sums = [[torch.zeros(8), torch.zeros(8)], [torch.zeros(16), torch.zeros(16)]]
    with torch.no_grad():
        for x, noise in cases:
            _, stats = _expected_block(blk, x, noise)
            blk(x, noise)
            for acc, (m, var) in zip(sums, stats):
                acc[0] += m
                acc[1] += var
    for m, acc in zip(norms, sums):
        assert m.accumulation_counter.item() == 3
        assert torch.allclose(m.stored_mean, acc[0], rtol=1e-5, atol=1e-6) and torch.allclose(m.stored_var, acc[1], rtol=1e-5, atol=1e-6)
    # eval() uses sums / counter
    blk.eval()
    x, noise = cases[0]
    with torch.no_grad():
        got = blk(x, noise)
        h = x
        for layer, conv, n, acc in ((blk.ch_a[0], blk.ch_a[2], noise[0], sums[0]), (blk.ch_a[3], blk.ch_a[5], noise[1], sums[1])):
            scale = torch.rsqrt(acc[1] / 3 + layer.bn.eps).view(1, -1, 1, 1) * (1 + layer.gain(n)).view(3, -1, 1, 1)
            h = conv(torch.relu(h * scale - ((acc[0] / 3).view(1, -1, 1, 1) * scale - layer.bias(n).view(3, -1, 1, 1))))
        want = h + blk.ch_b[0](x)
    assert (got - want).abs().max() <= 1e-5 * want.abs().max()
    norms[0].reset_stats()
    assert not norms[0].stored_mean.any() and not norms[0].stored_var.any() and norms[0].accumulation_counter.item() == 0


def test_the_other_ways_into_the_norm_no_longer_raise():
    torch.manual_seed(3)
    layer = A.LinearNoiseLayer(syn.network_opts(norm_G="sync:batch"), output_sz=8).train()       # (plain layers: the same weights at every call)
    x, noise = _block_case(8)
    f = ref.forward64(x, 1 + layer.gain(noise[0]).detach(), layer.bias(noise[0]).detach(), layer.bn.eps, False)
    want = f["y"].float()
    assert (layer(x, noise[0]) - want).abs().max() <= 1e-5 * want.abs().max()
    scale, shift = layer.affine(x, noise[0])
    assert (x * scale - shift - want).abs().max() <= 1e-5 * want.abs().max()
    pend = torch.randn(8)
    before = layer.bn.stored_mean.clone()
    sc, sh = layer.affine_bc(x, noise[0], pend)
    assert sc.shape == sh.shape == (3, 8) and (x * sc.view(3, 8, 1, 1) - sh.view(3, 8, 1, 1) - want).abs().max() <= 1e-5 * want.abs().max()
    assert torch.allclose(layer.bn.stored_mean, before * 0.9 + (f["mean"].float() + pend) * 0.1, rtol=1e-5, atol=1e-6)
    standing = A.BatchNorm_StandingStats(8).train()
    plain = ref.forward64(x, torch.ones(1, 8), torch.zeros(1, 8), 1e-5, False)["y"].float()
    assert (standing(x) - plain).abs().max() <= 1e-5 * plain.abs().max()
    with pytest.raises(RuntimeError, match="need the activation"):
        layer.bn.scale_shift(torch.ones(1, 8, 1, 1), torch.zeros(1, 8, 1, 1))


def test_the_switch(monkeypatch):
    """(the switch itself: tests/test_decoder_routing_cpu.py)"""
    monkeypatch.setattr(NT, "DECODER_NORM_TRAIN", NT.decoder_norm_train.from_env({}))
    assert NT.mode() == "hip" and A.decoder_norm_train is NT.decoder_norm_train
    # on the host both settings are the torch route: the same bits, and no entry point is called
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    x, gain, bias, _ = ref.inputs(2, 4, 3, 3)
    assert not NT.takes(x) and not NT.takes(x.double()) and not NT.takes(x[:, :3])
    out = []
    for m in ("hip", "torch"):
        layer = A.bn(4).train()
        with NT.decoder_norm_train(m):
            out.append((NT.batch_norm_train(x, gain, bias, layer, True), layer.stored_mean.clone(), layer.stored_var.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*out)) and not calls
