"""CPU-only: the host side of the discriminator's training pass (csrc/gan_train.hip, networks/gan_train.py, networks/discriminators.py and
losses/gan_loss.py with opt.isTrain): the C ABI of libpixelsynth_gan_train.so against its header and bindings, its refusals, the fp64
formulas of tests/_gan_train_ref.py against torch autograd, spectral normalisation in training against torch's own hook, one generator
and one discriminator step against the reference's outputs (tests/golden/gan_train.npz), the unchanged inference form, ten
adversarial steps, the switch and the aliases.  Everything here runs the torch route."""
import argparse
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _gan_train_ref as ref
from abi_util import ROOT, assert_library_matches_header
from pixelsynth_amd import _lib, _libraries, compat, synthetic as syn
from pixelsynth_amd.losses import DiscriminatorLoss, adversarial_step
from pixelsynth_amd.networks import discriminators as D, gan_train as GT

GOLD = os.path.join(ROOT, "tests", "golden")


def opts(**kw):
    o = dict(discriminator_losses="pix2pixHD", gan_mode="hinge", norm_D="spectralinstance", ndf=8, output_nc=3, no_ganFeat_loss=False,
             isTrain=True, lambda_feat=10.0, lr=1e-4, niter=100, niter_decay=10)
    o.update(kw)
    return argparse.Namespace(**o)


def test_the_registry_has_the_gan_train_library():
    entry = _libraries.LIBRARIES[-1]
    assert entry.name == "gan_train" and entry.so == "libpixelsynth_gan_train.so" and entry.headers == ("pixelsynth_gan_train.h",)
    assert entry.last_error == "ps_gan_train_last_error"
    assert [u for u, _ in entry.units] == ["gan_train.hip"] and entry.units[0][1] == _libraries.NO_CONTRACT
    protos = assert_library_matches_header("gan_train")
    assert set(protos) == set(_lib.GAN_TRAIN_PROTOS) == {
        "ps_gan_train_last_error", "ps_in_lrelu_forward_f32", "ps_in_lrelu_backward_f32", "ps_gan_feat_workspace_bytes",
        "ps_gan_feat_l1_f32", "ps_gan_feat_l1_backward_f32"}
    assert _lib.PROTOS["gan_train"] is _lib.GAN_TRAIN_PROTOS
    header = open(os.path.join(ROOT, "include", "pixelsynth_gan_train.h")).read()
    for name, value in (("RESIDENT_HW", ref.RESIDENT_HW), ("MAX_MAPS", ref.MAX_MAPS), ("WAVE_HW", ref.WAVE_HW), ("TILE", ref.TILE)):
        assert int(re.search(r"#define PS_GAN_TRAIN_%s (\d+)" % name, header).group(1)) == value
    assert GT.MAX_MAPS == ref.MAX_MAPS
    # the pinned library does not export what this one adds
    assert not any(hasattr(_lib.lib(), fn) for fn in protos)
    assert not any("gan" in s or "in_lrelu" in s for s in _lib.exported_symbols())
    # the forms of the header's table at their edges
    assert [ref.form(hw) for hw in (1, 256, 257, 2048, 2049, 3072, 3073, 4225, 8192, 8193)] == [
        ("wave", 4), ("wave", 4), ("wave", 8), ("wave", 32), ("workgroup", 12), ("workgroup", 12), ("workgroup", 16), ("workgroup", 20),
        ("workgroup", 32), ("stream", 0)]


def test_entry_points_refuse_before_anything_is_launched():
    L = _lib.library("gan_train")
    err = L.ps_gan_train_last_error
    p = torch.zeros(64).data_ptr()                     # (any non-null address: the arguments are refused before it is looked at)
    for bad in ((0, 4), (-2, 4), (3, 0), (3, -1)):
        assert L.ps_in_lrelu_forward_f32(p, bad[0], bad[1], 1e-5, 0.2, p, p, p, None, 0, None) != 0
        assert b"in_lrelu_forward" in err() and b"expected both >= 1" in err()
        assert L.ps_in_lrelu_backward_f32(p, p, p, p, bad[0], bad[1], 0.2, p, None, 0, None) != 0
        assert b"in_lrelu_backward" in err() and b"expected both >= 1" in err()
    for i in (0, 5, 6, 7):
        args = [p, 2, 4, 1e-5, 0.2, p, p, p, None, 0, None]
        args[i] = None
        assert L.ps_in_lrelu_forward_f32(*args) != 0 and b"in_lrelu_forward: null pointer" in err()
    for i in (0, 1, 2, 3, 7):
        args = [p, p, p, p, 2, 4, 0.2, p, None, 0, None]
        args[i] = None
        assert L.ps_in_lrelu_backward_f32(*args) != 0 and b"in_lrelu_backward: null pointer" in err()

    def tables(ns, ptr=p):
        n = len(ns)
        return (ctypes.c_void_p * n)(*[ptr] * n), (ctypes.c_longlong * n)(*ns), (ctypes.c_double * n)(*[1.0] * n)

    ws_of = L.ps_gan_feat_workspace_bytes
    assert ws_of(tables([1])[1], 1) == 256 and ws_of(tables([ref.TILE] * 16)[1], 16) == 256 and ws_of(tables([ref.TILE + 1] * 16)[1], 16) == 256
    assert ws_of(tables([ref.TILE * 20 + 1, 5])[1], 2) == 256 and ws_of(tables([ref.TILE * 32, 5])[1], 2) == 512
    for ns in ([], [0], [-4], [2 ** 40], [1] * 17):
        maps, halves, w = tables(ns or [1])
        assert ws_of(halves, len(ns)) == 0
        assert L.ps_gan_feat_l1_f32(maps, halves, w, len(ns), p, p, p, 1 << 20, None) != 0 and b"gan_feat_l1:" in err()
        assert L.ps_gan_feat_l1_backward_f32(maps, halves, w, len(ns), p, maps, None) != 0 and b"gan_feat_l1_backward:" in err()
    assert ws_of(None, 1) == 0
    maps, halves, w = tables([5, ref.TILE + 1])
    assert L.ps_gan_feat_l1_f32(maps, halves, w, 2, p, p, None, 24, None) != 0 and b"null pointer (workspace)" in err()
    assert L.ps_gan_feat_l1_f32(maps, halves, w, 2, p, p, p, 23, None) != 0 and b"workspace of 23 bytes, 24 needed" in err()
    assert L.ps_gan_feat_l1_f32(maps, halves, w, 2, p, p, p + 4, 64, None) != 0 and b"aligned to 16 bytes" in err()
    assert L.ps_gan_feat_l1_f32(maps, halves, w, 2, None, p, p, 64, None) != 0 and b"null pointer" in err()
    null_map = (ctypes.c_void_p * 2)(p, None)
    assert L.ps_gan_feat_l1_f32(null_map, halves, w, 2, p, p, p, 64, None) != 0 and b"null pointer (map 1)" in err()
    assert L.ps_gan_feat_l1_backward_f32(maps, halves, w, 2, p, null_map, None) != 0 and b"null pointer (gradient of map 1)" in err()
    # through the binding: a CPU tensor is refused by name before a stream is looked up
    z = torch.zeros(8)
    with pytest.raises(RuntimeError, match=r"ps_in_lrelu_forward_f32: args\[0\] is a CPU tensor.*no CPU fallback"):
        _lib.call("ps_in_lrelu_forward_f32", z, 2, 4, 1e-5, 0.2, z, z, z, None, 0)


def test_the_fp64_formulas_against_autograd():
    eps, slope = 1e-5, 0.2
    x, dy = ref.norm_inputs((2, 3, 5, 4), seed=1)
    f = ref.norm_forward64(x, eps, slope)
    want = F.leaky_relu(F.instance_norm(x.double(), eps=eps), slope)
    assert (f["y"] - want).abs().max() <= 1e-13
    g64 = ref.norm_autograd(x, dy, eps, slope, torch.float64)
    assert (ref.norm_backward64(x, dy, eps, slope) - g64).abs().max() <= 1e-12 * g64.abs().max()
    assert (ref.norm_backward64(x, dy, eps, slope, y=f["y"].float()) - g64).abs().max() <= 1e-12 * g64.abs().max()
    # what ships as the torch route is that composition, once differentiable in fp64
    assert torch.equal(GT.instance_norm_lrelu_train(x.double(), eps, slope), want)
    assert torch.autograd.gradcheck(lambda a: GT.instance_norm_lrelu_train(a, eps, slope), [x.double().requires_grad_()])
    # the bounds hold torch's own fp32 and not an error of one part in 10^5
    y32 = F.leaky_relu(F.instance_norm(x, eps=eps), slope)
    assert ref.check("fp32 y", y32, f["y"], ref.y_bound(x, f, eps)) <= 1.0
    assert ref.check("y off by 1e-5", y32 * (1 + 1e-5), f["y"], ref.y_bound(x, f, eps)) > 1.0
    bound, _ = ref.grad_bound(ref.norm_autograd(x, dy, eps, slope, torch.float32), g64)
    assert ref.check("dx without the m2 term", (g64 + 1e-3 * g64.abs().max()).float(), g64, bound) > 1.0
    # a single value: y = 0 and dx = 0
    one, done = ref.norm_inputs((2, 2, 1, 1))
    assert not ref.norm_forward64(one, eps, slope)["y"].any() and not ref.norm_backward64(one, done, eps, slope).any()
    # feature matching: the formula is the reference's loop; the gradient as the header rounds it is autograd's
    maps = ref.feat_maps([(4, 3, 5, 7), (4, 2, 3, 3), (2, 1, 1, 1)], seed=2)
    leaves = [m.clone().requires_grad_() for m in maps]
    total = GT.feature_matching(leaves, 5.0)
    per, tot64, mag = ref.feat_forward64(maps, [5.0] * 3)
    assert total.shape == (1,) and abs(total.item() - tot64) <= 4 * ref.U * mag
    manual = sum(F.l1_loss(m[: m.size(0) // 2], m[m.size(0) // 2:]) * 10.0 / 2 for m in maps)
    assert abs(total.item() - manual.item()) <= 4 * ref.U * mag
    total.backward(torch.tensor([0.7]))
    for leaf, want in zip(leaves, ref.feat_backward32(maps, [5.0] * 3, 0.7)):
        half = leaf.size(0) // 2
        assert not leaf.grad[half:].any() and (leaf.grad - want).abs().max() <= 4 * ref.U * want.abs().max()
        assert not leaf.grad[:half].reshape(-1)[::7].any()                          # the planted ties
    t2, pm = GT.feature_matching(maps, 5.0, per_map=True)
    assert torch.equal(t2, total.detach()) and np.allclose(pm.numpy(), per, rtol=1e-5)
    with pytest.raises(ValueError, match="no maps"):
        GT.feature_matching([], 1.0)


def test_spectral_norm_in_training_is_torchs_hook():
    """fp64, a 4096-term dot product (256 channels of 4 x 4): rounds near 5e-13, so 1e-12 relative"""
    torch.manual_seed(3)
    ours = D._SNConv(256, 8, 4, 2, 2, opts()).double().train()
    theirs = torch.nn.utils.spectral_norm(nn.Conv2d(256, 8, 4, 2, 2, bias=False)).double().train()
    with torch.no_grad():
        for name in ("weight_orig", "weight_u", "weight_v"):
            getattr(theirs, name).copy_(getattr(ours, name))
    x = torch.randn(2, 256, 6, 6, dtype=torch.float64)
    dy = torch.randn(2, 8, 4, 4, dtype=torch.float64)
    close = lambda a, b: (a - b).abs().max() <= 1e-12 * b.abs().max()
    for step in (1, 2):
        for m in (ours, theirs):
            m.weight_orig.grad = None
        a, b = ours(x), theirs(x)
        (a * dy).sum().backward()
        (b * dy).sum().backward()
        assert close(a, b) and close(ours.weight_u, theirs.weight_u) and close(ours.weight_v, theirs.weight_v), step
        assert close(ours.weight_orig.grad, theirs.weight_orig.grad), step
    # eval(), or isTrain false in train(): the stored vectors stay, and the arithmetic is today's
    u, v = ours.weight_u.clone(), ours.weight_v.clone()
    ours.eval()
    e = ours(x)
    assert torch.equal(ours.weight_u, u) and torch.equal(ours.weight_v, v)
    theirs.eval()
    assert close(e, theirs(x))
    frozen = D._SNConv(256, 8, 4, 2, 2, opts(isTrain=False)).double().train()
    frozen.load_state_dict(ours.state_dict())
    assert torch.equal(frozen(x), e) and torch.equal(frozen.weight_u, u) and D._SNConv(4, 4, 4, 2, 2).train().opt is None


def _mirror(seed, **kw):
    net = DiscriminatorLoss(opts(**kw)).train()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in syn.fill_state_dict(shapes, seed).items()}, strict=True)
    return net


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLD, "gan_train.npz"))


@pytest.mark.parametrize("S", [32, 64])
def test_both_steps_match_the_reference(fixture, S):
    """The reference's own DiscriminatorLoss in train() with isTrain (tests/golden/make_gan_train.py): a generator step, then a
    discriminator step.  Losses rtol 1e-5 / atol 1e-6, tensors rtol 1e-4 / atol 1e-5, as tests/test_scorers_cpu.py holds this mirror."""
    fx = fixture
    assert S in fx["sizes"]
    net = _mirror(int(fx["weight_seed"]))
    grid = int(fx["grid"])
    fake = torch.from_numpy(syn.image(int(fx["fake_seed"]) + S, 2, 3, S)).requires_grad_()
    real = torch.from_numpy(syn.image(int(fx["real_seed"]) + S, 2, 3, S))

    def recorded(tag):
        params = dict(net.named_parameters())
        for key in (k for k in fx.files if k.startswith(f"{tag}_grad_")):
            i, name = key[len(tag) + 6:].split("_", 1)
            got = params[f"netD.netD.discriminator_{i}.{name}"].grad.reshape(-1)[::grid].numpy()
            np.testing.assert_allclose(got, fx[key], rtol=1e-4, atol=1e-5, err_msg=key)
        us = [k for k in fx.files if k.startswith(f"{tag}_u_")]
        assert len(us) == 6
        for key in us:
            np.testing.assert_allclose(net.state_dict()[key[len(tag) + 3:]].numpy(), fx[key], rtol=1e-4, atol=1e-5, err_msg=key)

    g = net.run_generator_one_step(fake, real)
    assert set(g) == {"GAN", "GAN_Feat", "Total Loss"} and g["GAN"].shape == g["GAN_Feat"].shape == (1,)
    g["Total Loss"].mean().backward()
    for k, name in (("GAN", "GAN"), ("GAN_Feat", "GAN_Feat"), ("Total Loss", "total")):
        np.testing.assert_allclose(g[k].detach().reshape(-1).numpy(), fx[f"s{S}_g_{name}"], rtol=1e-5, atol=1e-6, err_msg=k)
    np.testing.assert_allclose(fake.grad[:, :, ::S // 8, ::S // 8].numpy(), fx[f"s{S}_g_dfake"], rtol=1e-4, atol=1e-5)
    recorded(f"s{S}_g")
    net.zero_grad()
    d = net.run_discriminator_one_step(fake.detach(), real)
    assert set(d) == {"D_Fake", "D_real", "Total Loss"}
    d["Total Loss"].mean().backward()
    for k, name in (("D_Fake", "D_Fake"), ("D_real", "D_real"), ("Total Loss", "total")):
        np.testing.assert_allclose(d[k].detach().reshape(-1).numpy(), fx[f"s{S}_d_{name}"], rtol=1e-5, atol=1e-6, err_msg=k)
    recorded(f"s{S}_d")


def test_the_training_entry_points_exist_and_carry_a_graph():
    """Fails on the parent commit: no run_generator_one_step, and discriminator mode ran under no_grad"""
    net = _mirror(5)
    assert hasattr(net, "run_generator_one_step") and hasattr(net, "get_optimizer")
    fake, real = (torch.from_numpy(syn.image(s, 1, 3, 32)) for s in (1, 2))
    g = net.run_generator_one_step(fake.requires_grad_(), real)
    assert g["Total Loss"].grad_fn is not None
    d = net.run_discriminator_one_step(fake, real)
    assert d["Total Loss"].grad_fn is not None
    opt = net.get_optimizer()
    assert isinstance(opt, torch.optim.Adam) and opt.defaults["lr"] == 2e-4 and opt.defaults["betas"] == (0, 0.9)
    assert sum(p.numel() for grp in opt.param_groups for p in grp["params"]) == sum(p.numel() for p in net.netD.parameters())
    with pytest.raises(ValueError, match="'generator' or 'discriminator'"):
        net.netD(fake, real, mode="both")
    # without the feature matching: the hinge term alone
    plain = _mirror(5, no_ganFeat_loss=True)
    g2 = plain.run_generator_one_step(fake, real)
    assert set(g2) == {"GAN", "Total Loss"} and torch.allclose(g2["GAN"], g["GAN"].detach(), rtol=1e-5, atol=1e-6)


def test_without_istrain_everything_is_the_inference_form():
    net = _mirror(5, isTrain=False)
    assert net.training and torch.is_grad_enabled()
    us = {k: v.clone() for k, v in net.state_dict().items() if k.endswith(("weight_u", "weight_v"))}
    fake, real = (torch.from_numpy(syn.image(s, 1, 3, 32)) for s in (1, 2))
    d = net.run_discriminator_one_step(fake.requires_grad_(), real)
    assert set(d) == {"D_Fake", "D_real", "Total Loss"} and all(v.grad_fn is None and not v.requires_grad for v in d.values())
    assert all(torch.equal(net.state_dict()[k], v) for k, v in us.items()) and len(us) == 12
    with pytest.raises(NotImplementedError, match="training is out of scope"):
        net.run_generator_one_step(fake, real)
    # the same numbers as the eval-mode scorer of the same weights, bit for bit (instance norm keeps no statistics)
    again = _mirror(5, isTrain=False).eval()
    assert all(torch.equal(d[k], v) for k, v in again.run_discriminator_one_step(fake, real).items())
    # and with isTrain, eval() under no_grad is that scorer too: no fused pair, no power iteration
    trained = _mirror(5).eval()
    with torch.no_grad():
        e = trained.run_discriminator_one_step(fake, real)
    assert all(torch.allclose(e[k], d[k], rtol=1e-6, atol=1e-7) for k in d) and all(torch.equal(trained.state_dict()[k], v) for k, v in us.items())


def test_ten_adversarial_steps():
    torch.manual_seed(0)
    netD = DiscriminatorLoss(opts(lr=1e-3)).train()
    gen = nn.Conv2d(3, 3, 3, padding=1)
    opt_G, opt_D = torch.optim.Adam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9)), netD.get_optimizer()
    src, gt = (torch.from_numpy(syn.image(s, 2, 3, 32)) for s in (7, 8))
    totals = []
    for _ in range(10):
        pred = torch.tanh(gen(src))
        l1 = F.l1_loss(pred, gt)
        before = [p.detach().clone() for p in list(gen.parameters()) + list(netD.parameters())]
        out = adversarial_step(netD, opt_G, opt_D, {"L1": l1, "Total Loss": l1}, pred, gt)
        assert set(out) == {"L1", "Total Loss", "GAN", "GAN_Feat", "D_Fake", "D_real"} and out["Total Loss"] is l1
        assert all(torch.isfinite(v).all() for v in out.values())
        # both sides moved: every parameter, but for the two last biases while every hinge is active (+1 of a fake and -1 of a real cancel)
        still = [torch.equal(a, b) for a, b in zip(before, list(gen.parameters()) + list(netD.parameters()))]
        assert not any(still[:2]) and sum(still) <= 2
        totals.append((out["D_Fake"] + out["D_real"]).mean().item())
    print("discriminator totals:", " ".join(f"{t:.4f}" for t in totals))
    assert totals[-1] < totals[0]


def test_the_switch(monkeypatch):
    monkeypatch.setattr(GT, "DISCRIMINATOR_TRAIN", GT.discriminator_train.from_env({}))
    assert GT.mode() == "hip" and GT.mode(opts(discriminator_train="torch")) == "torch"
    assert GT.discriminator_train.from_env({"PS_DISCRIMINATOR_TRAIN": "torch"}) == "torch"
    with GT.discriminator_train("torch"):
        assert GT.mode(opts(discriminator_train="hip")) == "torch"
    with pytest.raises(ValueError, match="'hip' or 'torch'"):
        GT.mode(opts(discriminator_train="triton"))
    # on the host both settings are the torch route: the same bits, and no entry point is called
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    x, _ = ref.norm_inputs((2, 3, 4, 5))
    maps = ref.feat_maps([(2, 3, 4, 4)])
    assert not GT.takes(x) and not GT.feat_takes(maps[0])
    out = []
    for m in ("hip", "torch"):
        with GT.discriminator_train(m):
            out.append((GT.instance_norm_lrelu_train(x), GT.feature_matching(maps, 2.0)))
    assert all(torch.equal(a, b) for a, b in zip(*out)) and not calls


def test_the_gan_aliases(monkeypatch):
    names = set(compat.GAN_ALIASES)
    assert names == {"models.losses.gan_loss", "models.networks.discriminators"}
    assert compat.TRAINING_ALIASES == {"models.losses.synthesis": "pixelsynth_amd.losses.synthesis"}
    saved = {k: sys.modules.get(k) for k in list(sys.modules) if k == "models" or k.startswith("models.")}
    for k in saved:
        monkeypatch.delitem(sys.modules, k)
    try:
        installed = compat.install_gan_aliases()
        assert set(installed) == names and compat.install_gan_aliases() == []
        from models.losses.gan_loss import DiscriminatorLoss as aliased
        import models.networks.discriminators as disc
        assert aliased is DiscriminatorLoss and disc is D
        assert "models.losses.synthesis" not in sys.modules
    finally:
        for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
            del sys.modules[k]
        sys.modules.update({k: v for k, v in saved.items() if v is not None})
