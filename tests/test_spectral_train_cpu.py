"""CPU-only: the host side of the batched spectral normalisation (csrc/spectral_train.hip, networks/spectral_train.py): the registry
entry and the C ABI of libpixelsynth_spectral_train.so against its header and bindings, the plan (a pure host function) against its
mirrors, its refusals, the switch and the training context, the fall-back to the hook on the host, and the fp64 mirror and the bounds of
tests/_spectral_ref.py against torch's hook, autograd and a simulation of the kernels' roundings."""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn
from torch.nn.utils.spectral_norm import SpectralNorm

import _spectral_ref as ref
from _forward_train_util import train_opts
from abi_util import ROOT, assert_library_matches_header
from pixelsynth_amd import _lib, _libraries, training
from pixelsynth_amd.networks import architectures as arch, conv_routes, discriminators as D, routing, spectral_train as ST


def test_the_registry_has_the_spectral_train_library():
    names = [e.name for e in _libraries.LIBRARIES]
    at = names.index("spectral_train")
    entry = _libraries.LIBRARIES[at]
    assert names[-1] == "gan_train" and at < len(names) - 1 and list(_lib.PROTOS)[at] == "spectral_train" and list(_lib.PROTOS) == names
    assert entry.so == "libpixelsynth_spectral_train.so" and entry.headers == ("pixelsynth_spectral_train.h",)
    assert entry.last_error == "ps_spectral_train_last_error"
    assert [u for u, _ in entry.units] == ["spectral_train.hip"] and entry.units[0][1] == _libraries.NO_CONTRACT
    protos = assert_library_matches_header("spectral_train")
    assert set(protos) == set(_lib.SPECTRAL_TRAIN_PROTOS) == {
        "ps_spectral_train_last_error", "ps_spectral_table_bytes", "ps_spectral_plan", "ps_spectral_workspace_bytes",
        "ps_spectral_forward_f32", "ps_spectral_backward_f32"}
    assert _lib.PROTOS["spectral_train"] is _lib.SPECTRAL_TRAIN_PROTOS
    header = open(os.path.join(ROOT, "include", "pixelsynth_spectral_train.h")).read()
    for name, value, mine in (("MAX_LAYERS", ref.MAX_LAYERS, ST.MAX_LAYERS), ("PART_ROWS", ref.PART_ROWS, ST.PART_ROWS),
                              ("TILE", ref.TILE, ST.TILE), ("FORWARD_LAUNCHES", ref.FORWARD_LAUNCHES, ST.FORWARD_LAUNCHES),
                              ("BACKWARD_LAUNCHES", ref.BACKWARD_LAUNCHES, ST.BACKWARD_LAUNCHES)):
        assert int(re.search(r"#define PS_SPECTRAL_%s (\d+)" % name, header).group(1)) == value == mine
    # the pinned library does not export what this one adds; every call of the package goes through _lib.call
    assert not any(hasattr(_lib.lib(), fn) for fn in protos)
    assert not any("spectral" in s for s in _lib.exported_symbols())
    source = open(os.path.join(ROOT, "pixelsynth_amd", "networks", "spectral_train.py")).read()
    assert set(re.findall(r"\"(ps_spectral_\w+)\"", source)) == set(protos) - {"ps_spectral_train_last_error"}
    assert not re.search(r"_lib\.(library|lib)\(", source)


def _plan(shapes, inter=None, iterate=None, eps=None, base=4096):
    """ps_spectral_plan on made-up addresses (a pure host function) -> (rc, table, elem, row, col)"""
    L = _lib.library("spectral_train")
    n = len(shapes)
    ptr = (ctypes.c_void_p * max(n, 1))(*[base + 256 * k for k in range(max(n, 1))])
    ints = lambda vals: (ctypes.c_int * max(n, 1))(*vals) if n else (ctypes.c_int * 1)()
    table = ctypes.create_string_buffer(L.ps_spectral_table_bytes())
    offs = [(ctypes.c_longlong * (n + 1))() for _ in range(3)]
    rc = L.ps_spectral_plan(ptr, ptr, ptr, ints([s[0] for s in shapes]), ints([s[1] for s in shapes]), ints(inter or [1] * n),
                            ints(iterate or [1] * n), (ctypes.c_float * max(n, 1))(*(eps or [1e-12] * n)), n, table, len(table), *offs)
    return (rc, table) + tuple(list(o) for o in offs)


def test_the_plan_and_the_workspace_against_their_mirrors():
    L = _lib.library("spectral_train")
    shapes = ref.SHAPES + ref.BOUNDARY_SHAPES
    rc, table, elem, row, col = _plan(shapes)
    assert rc == 0
    up4 = lambda n: -(-n // 4) * 4
    want_elem, want_row, want_col = [0], [0], [0]
    for R, C in shapes:
        want_elem.append(want_elem[-1] + up4(R * C))
        want_row.append(want_row[-1] + R)
        want_col.append(want_col[-1] + up4(C))
    assert (elem, row, col) == (want_elem, want_row, want_col)
    assert L.ps_spectral_workspace_bytes(table) == ref.workspace_bytes(shapes) == ST.workspace_bytes(shapes)
    for R, C in shapes:         # a layer's share does not depend on its neighbours: alone it has the same plan
        assert ST.plan(R, C) == ref.plan(R, C)
        assert L.ps_spectral_workspace_bytes(_plan([(R, C)])[1]) == ref.workspace_bytes([(R, C)])
    # the plan at its edges: parts of 16 rows, groups of four rows, tiles of 4096 values
    assert [ref.plan(*s) for s in ((16, 64), (17, 64), (4, 9), (5, 7), (64, 64), (64, 65), (512, 4608))] == [
        (1, 4, 1), (2, 5, 1), (1, 1, 1), (1, 2, 1), (4, 16, 1), (4, 16, 2), (32, 128, 576)]
    # the full configuration's largest table stays below the cap: the decoder's 54
    assert 54 <= ref.MAX_LAYERS and _plan([(8, 20)] * ref.MAX_LAYERS)[0] == 0


def test_entry_points_refuse_before_anything_is_launched():
    L = _lib.library("spectral_train")
    err = L.ps_spectral_train_last_error
    assert _plan([])[0] != 0 and b"n_layers = 0, expected 1 .. 64" in err()
    assert _plan([(8, 20)] * 65)[0] != 0 and b"n_layers = 65" in err()
    for bad in ((0, 4), (4, 0), (-1, 4), (65536, 32768)):
        assert _plan([(3, 3), bad])[0] != 0 and b"spectral_plan: layer 1 is" in err()
    assert _plan([(3, 12)], inter=[5])[0] != 0 and b"interleave = 5, expected a divisor of C = 12" in err()
    assert _plan([(3, 12)], inter=[0])[0] != 0 and b"interleave" in err()
    assert _plan([(3, 12)], inter=[4])[0] == 0
    assert _plan([(3, 12)], eps=[0.0])[0] != 0 and b"eps = 0, expected > 0" in err()
    assert _plan([(3, 12)], base=4098)[0] != 0 and b"not aligned to 4 bytes" in err()
    assert _plan([(3, 12)], base=0)[0] != 0 and b"null pointer (layer 0)" in err()
    rc, table, *_ = _plan([(3, 12), (5, 7)])
    small = ctypes.create_string_buffer(16)
    one, p = (ctypes.c_int * 1)(3), (ctypes.c_void_p * 1)(4096)
    assert L.ps_spectral_plan(p, p, p, one, one, one, one, (ctypes.c_float * 1)(1e-12), 1, small, 16, None, None, None) != 0
    assert b"a table of 16 bytes" in err()
    # the queued calls: a table that the plan did not fill, a stale image, the workspace
    a = torch.zeros(64).data_ptr()
    junk = ctypes.create_string_buffer(len(table))
    assert L.ps_spectral_workspace_bytes(junk) == 0 and L.ps_spectral_workspace_bytes(None) == 0
    assert L.ps_spectral_forward_f32(junk, a, a, a, a, a, a, 1 << 20, None) != 0 and b"not a table ps_spectral_plan filled" in err()
    edited = ctypes.create_string_buffer(table.raw)
    edited[40] = bytes([edited.raw[40] ^ 1])
    assert L.ps_spectral_backward_f32(edited, a, p, a, a, a, a, a, a, 1 << 20, None) != 0 and b"not a table" in err()
    need = L.ps_spectral_workspace_bytes(table)
    assert L.ps_spectral_forward_f32(table, None, a, a, a, a, a, need, None) != 0 and b"null pointer (table_device)" in err()
    assert L.ps_spectral_forward_f32(table, a, a, a, a, a, None, need, None) != 0 and b"null pointer (workspace)" in err()
    assert L.ps_spectral_forward_f32(table, a, a, a, a, a, a, need - 1, None) != 0 and b"bytes, %d needed" % need in err()
    assert L.ps_spectral_forward_f32(table, a, a, a, a, a, a + 4, need, None) != 0 and b"aligned to 16 bytes" in err()
    assert L.ps_spectral_forward_f32(table, a, None, a, a, a, a, need, None) != 0 and b"spectral_forward: null pointer" in err()
    assert L.ps_spectral_forward_f32(table, a, a + 4, a, a, a, a, need, None) != 0 and b"w_sn and v_saved must be aligned" in err()
    g2 = (ctypes.c_void_p * 2)(a, a + 2)
    assert L.ps_spectral_backward_f32(table, a, g2, a, a, a, a, a, a, need, None) != 0 and b"gradient of layer 1 is not aligned" in err()
    assert L.ps_spectral_backward_f32(table, a, None, a, a, a, a, a, a, need, None) != 0 and b"spectral_backward: null pointer" in err()
    # through the binding: a CPU tensor is refused by name before a stream is looked up
    z = torch.zeros(8)
    with pytest.raises(RuntimeError, match=r"ps_spectral_forward_f32: args\[1\] is a CPU tensor.*no CPU fallback"):
        _lib.call("ps_spectral_forward_f32", 0, z, z, z, z, z, z, 0)


def test_the_switch(monkeypatch):
    monkeypatch.setattr(ST, "SPECTRAL_TRAIN", ST.spectral_train.from_env({}))
    opt = lambda **kw: train_opts(**kw)
    assert ST.mode() == "torch" and ST.mode(opt(spectral_train="hip")) == "hip" and ST.spectral_train.default == "torch"
    assert ST.spectral_train.from_env({"PS_SPECTRAL_TRAIN": "hip"}) == "hip" and ST.spectral_train.env == "PS_SPECTRAL_TRAIN"
    with ST.spectral_train("hip"):
        assert ST.mode(opt(spectral_train="torch")) == "hip"
        with ST.spectral_train("torch"):
            assert ST.mode() == "torch"
        assert ST.mode() == "hip"
    assert ST.mode() == "torch"
    with pytest.raises(ValueError, match="'hip' or 'torch'"):
        ST.mode(opt(spectral_train="triton"))
    with pytest.raises(ValueError, match="'hip' or 'torch'"):
        ST.spectral_train("cuda")
    # active(): the "hip" route, and grad mode or train() -- not where the eval-mode cache is taken
    net = nn.Linear(2, 2)
    with ST.spectral_train("hip"):
        assert ST.active(net) and ST.active(net.eval())
        with torch.no_grad():
            assert not ST.active(net) and ST.active(net.train())
    assert not ST.active(net)


def test_the_training_context_stacks_the_switch():
    assert len(training.HIP_ROUTES) == 5 and ST.spectral_train not in [s for s, _ in training.HIP_ROUTES]
    with training.hip_routes() as plain:
        assert ST.spectral_train.forced() is None
    with training.hip_routes_with_spectral() as forced:
        assert forced == dict(plain, spectral_train="hip") and ST.mode() == "hip" and D.disc_conv.discriminator_conv_train.forced() is None
    with training.hip_routes_with_spectral(discriminator=True) as forced:
        assert forced == dict(plain, spectral_train="hip", discriminator_conv_train="f16")
    assert ST.spectral_train.forced() is None


def _decoder(seed=0):
    torch.manual_seed(seed)
    return arch.get_decoder(train_opts()).train()


def _spies(monkeypatch):
    hooks, calls = [], []
    real_hook, real_call = SpectralNorm.compute_weight, _lib.call
    monkeypatch.setattr(SpectralNorm, "compute_weight", lambda self, m, do_power_iteration: (hooks.append(do_power_iteration), real_hook(self, m, do_power_iteration))[1])
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real_call(name, *a, **k))[1])
    return hooks, calls


def test_on_the_host_hip_is_the_hook_bit_for_bit(monkeypatch):
    hooks, calls = _spies(monkeypatch)
    x, mask = torch.randn(1, 3, 16, 16), torch.rand(1, 16, 16) > 0.5
    noise = [torch.randn(1, arch.NOISE_SZ) for _ in range(16)]
    out = {}
    for m in ("torch", "hip"):
        net = _decoder()
        assert len(ST.sn_modules(net)) == 54 and not ST.normalise(ST.sn_modules(net))       # nothing on the host is taken
        del hooks[:]
        with ST.spectral_train(m):
            y = net(x, mask, noise)
            y.square().sum().backward()
        out[m] = (y.detach(), [p.grad for p in net.parameters()], [b.clone() for b in net.buffers()], len(hooks))
        assert not any(routing.has_pending(mod) for mod in net.modules())
    for a, b in zip(out["torch"][:3], out["hip"][:3]):
        assert all(torch.equal(s, t) for s, t in zip(a, b)) if isinstance(a, list) else torch.equal(a, b)
    assert out["torch"][3] == out["hip"][3] == 54 and not [c for c in calls if "spectral" in c]
    # the discriminator and fp64 the same way
    disc = D.define_D(train_opts()).double().train()
    img = torch.randn(1, 3, 32, 32, dtype=torch.float64)
    twin = copy.deepcopy(disc)
    with ST.spectral_train("hip"):
        a = disc(img)
    b = twin(img)
    assert all(torch.equal(s, t) for p, q in zip(a, b) for s, t in zip(p, q))
    assert all(torch.equal(s, t) for s, t in zip(disc.buffers(), twin.buffers()))


def test_a_pending_weight_is_taken_once_and_never_stale():
    torch.manual_seed(1)
    conv = nn.utils.spectral_norm(nn.Conv2d(3, 4, 3, padding=1)).train()
    x = torch.randn(1, 3, 5, 5)
    fake = torch.full_like(conv.weight_orig, 0.5)
    routing.leave_pending(conv, fake)
    assert routing.has_pending(conv)
    w = conv_routes._plain_conv_weight(conv, x)
    assert w is fake and conv.weight is fake and not routing.has_pending(conv)       # taken, assigned as the hook assigns it
    u = conv.weight_u.clone()
    again = conv_routes._plain_conv_weight(conv, x)                                   # nothing pending: the hook, one power iteration
    assert again is not fake and not torch.equal(conv.weight_u, u)
    # a weight of another state is dropped: an optimiser step, or the hook itself, came between
    routing.leave_pending(conv, fake)
    with torch.no_grad():
        conv.weight_orig.mul_(1.0)
    assert conv_routes._plain_conv_weight(conv, x) is not fake and not routing.has_pending(conv)
    # _conv_split and Unet._conv reach a pending weight without the hook's second iteration
    routing.leave_pending(conv, fake)
    u = conv.weight_u.clone()
    y, bias = conv_routes._conv_split(conv, x)
    assert bias is None and torch.equal(conv.weight_u, u) and torch.equal(y, torch.nn.functional.conv2d(x, fake, conv.bias, padding=1))
    routing.leave_pending(conv, fake)
    assert torch.equal(arch.Unet._conv(conv, x), y) and torch.equal(conv.weight_u, u)
    sn = D._SNConv(3, 4, 4, 2, 1, train_opts()).train()
    fake = torch.full_like(sn.weight_orig, 0.25)
    routing.leave_pending(sn, fake)
    u = sn.weight_u.clone()
    assert sn.weight() is fake and torch.equal(sn.weight_u, u) and sn.weight() is not fake and not torch.equal(sn.weight_u, u)
    # what normalise() takes: it says no to everything here on the host, and to hooks outside its scope anywhere
    assert ST._layer(conv) is None and ST._layer(sn) is None and ST._layer(nn.Conv2d(3, 4, 3)) is None
    assert ST._interleave(torch.empty(4, 3, 3, 3)) == 1 and ST._interleave(torch.empty(4, 3, 3, 3).to(memory_format=torch.channels_last)) == 3
    assert ST._interleave(torch.empty(4, 3, 1, 1).to(memory_format=torch.channels_last)) == 1 and ST._interleave(torch.empty(4, 6)[:, ::2]) is None


@pytest.mark.parametrize("iterate", [True, False])
def test_the_fp64_mirror_is_torchs_hook_and_its_autograd(iterate):
    for R, C in ref.SHAPES:
        W, u, v = ref.layer_inputs(R, C, seed=3)
        lin = nn.utils.spectral_norm(nn.Linear(C, R, bias=False)).double().train(iterate)
        with torch.no_grad():
            lin.weight_orig.copy_(W), lin.weight_u.copy_(u), lin.weight_v.copy_(v)
        f = ref.forward64(W, u, v, iterate)
        lin(torch.zeros(1, C, dtype=torch.float64))                  # the hook: lin.weight, and u / v in place
        G = torch.randn(R, C, generator=torch.Generator().manual_seed(R))
        (lin.weight * G.double()).sum().backward()
        scale = lambda t: 1e-13 * t.abs().max()
        assert (lin.weight.detach() - f["w"]).abs().max() <= scale(f["w"])
        assert (lin.weight_u - f["u"]).abs().max() <= 1e-13 and (lin.weight_v - f["v"]).abs().max() <= 1e-13
        dW = ref.backward64(f, G)
        assert (lin.weight_orig.grad - dW).abs().max() <= 1e-12 * dW.abs().max()
        assert (ref.autograd(W, u, v, iterate, G, torch.float64) - dW).abs().max() <= 1e-12 * dW.abs().max()
        # hook32 is the hook's own fp32 arithmetic, bit for bit
        lin32 = nn.utils.spectral_norm(nn.Linear(C, R, bias=False)).train(iterate)
        with torch.no_grad():
            lin32.weight_orig.copy_(W), lin32.weight_u.copy_(u), lin32.weight_v.copy_(v)
        lin32(torch.zeros(1, C))
        h = ref.hook32(W, u, v, iterate)
        assert torch.equal(h["w"], lin32.weight.detach()) and torch.equal(h["u"], lin32.weight_u) and torch.equal(h["v"], lin32.weight_v)


@pytest.mark.parametrize("iterate", [True, False])
def test_the_bounds_hold_the_roundings_and_not_a_wrong_formula(iterate):
    worst = 0.0
    for R, C in ref.SHAPES + ref.BOUNDARY_SHAPES:
        W, u, v = ref.layer_inputs(R, C, seed=5)
        f, h, sim = ref.forward64(W, u, v, iterate), ref.hook32(W, u, v, iterate), ref.simulate(W, u, v, iterate)
        e = ref.forward_errors(W, u, v, iterate, f)
        for k in ("v", "u", "sigma", "w"):
            bound = ref.bounded(e[k], h[k], f[k])
            worst = max(worst, ref.check(f"{R}x{C} {k}", sim[k], f[k], bound))
            if iterate:       # a value off by one part in 10^5 is outside (random u, v that do not iterate: sigma is a small sum of cancelling terms)
                assert ref.check(f"{R}x{C} {k} off", sim[k].double() * (1 + 1e-5), f[k], bound) > 1.0
        for kind in ("randn", "correlated"):
            G = torch.randn(R, C, generator=torch.Generator().manual_seed(C))
            G = G if kind == "randn" else f["w"].float() + 0.1 * G
            dW = ref.backward64(f, G)
            bound = ref.bounded(ref.backward_error(f, e, G, dW), ref.autograd(W, u, v, iterate, G, torch.float32), dW)
            worst = max(worst, ref.check(f"{R}x{C} dW {kind}", ref.simulate_backward(sim, G), dW, bound))
            if kind == "correlated" and R * C > 1:   # the u v^T term dropped: far outside
                assert ref.check(f"{R}x{C} dW without u v^T", G.double() / f["sigma"], dW, bound) > 10.0
    assert worst <= 1.0
