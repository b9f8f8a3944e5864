"""GPU: the discriminator's 4 x 4 convolution on the fp16 matrix pipe (csrc/disc_conv.hip behind include/pixelsynth_disc_conv.h, the
autograd Function of networks/disc_conv.py, _SNConv's route).

Operator level: the index walk bit for bit on small integers, the accuracy under the two rules of tests/_disc_conv_ref.py (with small
gradients too), a frame alone and in a batch, two runs, the overflow words.  Network level: the discriminator at ndf = 64 against its fp64
twin on the host (the construction and the bounds of tests/test_gan_train_gpu.py), the routes against each other, ten adversarial steps,
and the parent route's bits in eval mode and under no_grad.  Every check prints its error / bound.
"""
import argparse
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _disc_conv_ref as ref
import _gan_train_ref as gref
from pixelsynth_amd import _lib, synthetic as syn
from pixelsynth_amd.losses import DiscriminatorLoss, adversarial_step
from pixelsynth_amd.networks import disc_conv as DC, f16x3, gan_train as GT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(x, w, g, stride, need=(True, True)):
    """conv4x4_train forward and backward on the device -> y, grad_x, grad_weight (None where not needed)"""
    xd, wd = x.to(DEV).requires_grad_(need[0]), w.to(DEV).requires_grad_(need[1])
    assert DC.takes(xd, wd, stride)
    y = DC.conv4x4_train(xd, wd, stride)
    assert type(y.grad_fn).__name__ == "_DiscConvBackward" and y.is_contiguous()
    y.backward(g.to(DEV))
    return y.detach(), xd.grad, wd.grad


def _clear():
    f16x3.flag(DEV).zero_()
    f16x3.grad_flag(DEV).zero_()


def _flags():
    return int(f16x3.flag(DEV).item()), int(f16x3.grad_flag(DEV).item())


# ---------------------------------------------------------------- the index walk, bit for bit
def integers_bit_for_bit(shape, run=_run, operands=None):
    """The body of test_integers_bit_for_bit (tests/test_disc_routes_gpu.py runs its cases through it too, with a `run` of its own: the
    entry points with their outputs inside rims; and with `operands`, the six tensors of ref.integers times powers of two)"""
    x, w, g, y64, gx64, gw64 = operands or ref.integers(shape)
    _clear()
    y, gx, gw = run(x, w, g, shape[5])
    assert tuple(y.shape) == ref.out_shape(*shape)
    assert torch.equal(y.cpu(), y64), f"y: {(y.cpu() != y64).sum().item()} of {y64.numel()} differ"
    assert torch.equal(gx.cpu(), gx64), f"grad_x: {(gx.cpu() != gx64).sum().item()} of {gx64.numel()} differ"
    assert torch.equal(gw.cpu(), gw64), f"grad_weight: {(gw.cpu() != gw64).sum().item()} of {gw64.numel()} differ"
    assert _flags() == (0, 0)
    # every output twice: the same bits; and each gradient alone (needs_input_grad) is the same gradient
    y2, gx2, gw2 = run(x, w, g, shape[5])
    assert torch.equal(y, y2) and torch.equal(gx, gx2) and torch.equal(gw, gw2)
    _, gx3, none = run(x, w, g, shape[5], need=(True, False))
    assert none is None and torch.equal(gx3, gx)
    _, none, gw3 = run(x, w, g, shape[5], need=(False, True))
    assert none is None and torch.equal(gw3, gw)


@pytest.mark.parametrize("shape", ref.ALL_SHAPES, ids=str)
def test_integers_bit_for_bit(shape):
    integers_bit_for_bit(shape)


# ---------------------------------------------------------------- accuracy
@functools.lru_cache(maxsize=None)
def _reference(shape, small):
    x, w, g = ref.small_gradients(shape) if small else ref.inputs(shape)
    return x, w, g, ref.reference(x, w, g, shape[5])


def accuracy_under_both_rules(shape, run=_run):
    """The body of test_accuracy_under_both_rules (tests/test_disc_routes_gpu.py runs its cases through it too)"""
    x, w, g, r = _reference(shape, False)
    _clear()
    y, gx, gw = run(x, w, g, shape[5])
    ref.check(f"{shape} y", y, r.y)
    ref.check(f"{shape} grad_x", gx, r.x)
    ref.check(f"{shape} grad_weight", gw, r.weight)
    assert _flags() == (0, 0)
    y2, gx2, gw2 = run(x, w, g, shape[5])
    assert torch.equal(y, y2) and torch.equal(gx, gx2) and torch.equal(gw, gw2)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_accuracy_under_both_rules(shape):
    accuracy_under_both_rules(shape)


@pytest.mark.parametrize("shape", [ref.SHAPES[3], ref.SHAPES[4]], ids=str)
def test_small_gradients_keep_rule_2(shape):
    x, w, g, r = _reference(shape, True)
    assert r.sg >= 2.0 ** 30                                     # what the scaling is for
    y, gx, gw = _run(x, w, g, shape[5])
    assert float(DC._DiscConv.last_scale2[0].item()) == r.sg and float(DC._DiscConv.last_scale2[1].item()) == 1.0 / r.sg
    ref.check(f"{shape} small grad_x", gx, r.x)
    ref.check(f"{shape} small grad_weight", gw, r.weight)


# ---------------------------------------------------------------- invariance
@pytest.mark.parametrize("stride", [1, 2])
def test_a_frame_alone_and_in_a_batch(stride):
    x, w, g = ref.inputs((3, 64, 128, 33, 34, stride), seed=3)
    y, gx, _ = _run(x, w, g, stride)
    y1, gx1, _ = _run(x[1:2], w, g[1:2], stride)
    assert torch.equal(y[1:2], y1) and torch.equal(gx[1:2], gx1)


# ---------------------------------------------------------------- overflow
def test_overflow_words():
    shape = (2, 64, 64, 9, 11, 2)
    x, w, g = ref.inputs(shape, seed=4)
    for bad in (7e4, float("nan")):
        xb = x.clone()
        xb[1, 5, 3, 4] = bad
        _clear()
        xd, wd = xb.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
        y = DC.conv4x4_train(xd, wd, 2)
        assert _flags() == (1, 0), bad                           # the forward raises the activations' word alone
        _clear()
        y.backward(g.to(DEV))                                    # a clean grad_y: x is met again by the grad_weight pass
        assert _flags() == (1, 0), bad
        assert torch.isfinite(xd.grad).all()
    gb = g.clone()
    gb[0, 3, 2, 2] = float("nan")
    _clear()
    y, gx, gw = _run(x, w, gb, 2)
    assert _flags() == (0, 1)                                    # a gradient that is not finite: its own word, flag stays clear
    assert not torch.isfinite(gx).all() and not torch.isfinite(gw).all()
    _clear()
    y, gx, gw = _run(x, w, torch.zeros_like(g), 2)
    assert DC._DiscConv.last_scale2.tolist() == [1.0, 1.0]
    assert torch.isfinite(gx).all() and torch.isfinite(gw).all() and not gx.any() and not gw.any() and _flags() == (0, 0)


# ---------------------------------------------------------------- the whole network
def _opts(ndf, **kw):
    o = dict(discriminator_losses="pix2pixHD", gan_mode="hinge", norm_D="spectralinstance", ndf=ndf, output_nc=3, no_ganFeat_loss=False,
             isTrain=True, lambda_feat=10.0, lr=1e-3, niter=100, niter_decay=10)
    o.update(kw)
    return argparse.Namespace(**o)


def _net(ndf, seed=11, **kw):
    net = DiscriminatorLoss(_opts(ndf, **kw)).train()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in syn.fill_state_dict(shapes, seed).items()}, strict=True)
    return net


KINK = 2.0 ** -16
SEEDS = (47, 48)      # the fake and the real image of tests/test_gan_train_gpu.py's ndf = 64 case: no normalised value near the kink


def _both_steps(net, fake, real):
    out = {}
    fake = fake.clone().requires_grad_()
    g = net.run_generator_one_step(fake, real)
    g["Total Loss"].mean().backward()
    out.update({f"g/{k}": v.detach().clone() for k, v in g.items()})
    out["g/dfake"] = fake.grad.clone()
    out.update({f"g/grad/{k}": p.grad.clone() for k, p in net.named_parameters()})
    net.zero_grad()
    d = net.run_discriminator_one_step(fake.detach(), real)
    d["Total Loss"].mean().backward()
    out.update({f"d/{k}": v.detach().clone() for k, v in d.items()})
    out.update({f"d/grad/{k}": p.grad.clone() for k, p in net.named_parameters()})
    return out


def test_the_network_against_its_fp64_twin(monkeypatch):
    """Both modes of DiscriminatorLoss (a generator step, a discriminator step) of the multiscale discriminator at ndf = 64 on one pair
    of 32 x 32 under "f16": losses, the gradient to the fake image and every parameter's gradient under the twin test's bound,
    4 max(|host fp32 - fp64|, 1e-6 max |fp64|)."""
    net = _net(64)
    twin64, twin32 = copy.deepcopy(net).double(), copy.deepcopy(net)
    fake, real = (torch.from_numpy(syn.image(s, 1, 3, 32)) for s in SEEDS)
    undecided, formula = [], GT.norm_formula

    def spy(x, eps=1e-5, slope=0.2):
        undecided.append(int((gref.norm_forward64(x.detach(), eps, slope)["v"].abs() < KINK).sum()))
        return formula(x, eps, slope)
    monkeypatch.setattr(GT, "norm_formula", spy)
    want = _both_steps(twin64, fake.double(), real.double())
    monkeypatch.setattr(GT, "norm_formula", formula)
    assert len(undecided) == 12 and not any(undecided), undecided
    host32 = _both_steps(twin32, fake, real)
    calls, real_call = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real_call(name, *a, **k))[1])
    net = net.to(DEV)
    _clear()
    with GT.discriminator_train("hip"), DC.discriminator_conv_train("f16"):
        got = _both_steps(net, fake.to(DEV), real.to(DEV))
        # the five maps are dense NCHW, behind _InLrelu, which is behind _DiscConv
        maps = net.netD.netD.discriminator_0(fake.to(DEV))
    assert len(maps) == 5 and all(m.is_contiguous() and GT.takes(m) for m in maps)
    for m in maps[1:4]:
        assert type(m.grad_fn).__name__ == "_InLreluBackward"
        assert type(m.grad_fn.next_functions[0][0]).__name__ == "_DiscConvBackward"
    # three convolutions and three norms per discriminator, two discriminators, two forwards and two backwards (and the maps' forward)
    assert calls.count("ps_disc_conv_forward_f16x3") == 12 + 3 and calls.count("ps_disc_conv_backward_f16x3") == 12
    assert calls.count("ps_in_lrelu_forward_f32") == 12 + 3 and calls.count("ps_in_lrelu_backward_f32") == 12
    assert calls.count("ps_gan_feat_l1_f32") == 1 and calls.count("ps_gan_feat_l1_backward_f32") == 1
    assert _flags()[0] == 0
    assert set(got) == set(want) and len(got) == 7 + 2 * len(list(net.parameters()))
    worst = 0.0
    for k in want:
        bound, _ = gref.grad_bound(host32[k], want[k])
        worst = max(worst, gref.check(k, got[k], want[k], bound))
    print(f"ndf = 64 under f16: largest error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("multiscale", [False, True], ids=["n_layer", "multiscale"])
def test_the_routes_agree(multiscale):
    fake, real = (torch.from_numpy(syn.image(s, 1, 3, 32)).to(DEV) for s in (23, 24))
    if not multiscale:      # one NLayerDiscriminator: its five maps under both routes
        net = _net(64).eval().to(DEV).netD.netD.discriminator_0      # (eval: no power iteration between the two calls)
        with DC.discriminator_conv_train("f16"):
            a = net(fake)
        with DC.discriminator_conv_train("torch"):
            b = net(fake)
        assert type(a[1].grad_fn.next_functions[0][0]).__name__ == "_DiscConvBackward"
        assert type(b[1].grad_fn.next_functions[0][0]).__name__ != "_DiscConvBackward"
        for i, (u, v) in enumerate(zip(a, b)):
            err, top = (u - v).abs().max().item(), v.abs().max().item()
            print(f"map {i}: max |f16 - torch| {err:.3e} of {top:.3e}")
            assert err <= 1e-5 * max(top, 1.0)
        return
    out = {}
    for route in ("f16", "torch"):
        net = _net(64, seed=8).to(DEV)
        with DC.discriminator_conv_train(route):
            g = net.run_generator_one_step(fake, real)
            d = net.run_discriminator_one_step(fake, real)
        out[route] = {**{f"g/{k}": v for k, v in g.items()}, **{f"d/{k}": v for k, v in d.items()}}
    for k, v in out["f16"].items():
        w = out["torch"][k]
        print(k, v.item(), w.item(), f"difference {(v - w).abs().item():.3e}")
        assert (v - w).abs().item() <= 1e-5 * max(w.abs().item(), 1.0), k
    # the option selects the route like the switch
    net = _net(64, discriminator_conv_train="f16").to(DEV)
    m = net.netD.netD.discriminator_0(fake)[1]
    assert type(m.grad_fn.next_functions[0][0]).__name__ == "_DiscConvBackward"


def test_ten_adversarial_steps_on_the_device():
    torch.manual_seed(0)
    netD = DiscriminatorLoss(_opts(64)).train().to(DEV)
    gen = nn.Conv2d(3, 3, 3, padding=1).to(DEV)
    opt_G, opt_D = torch.optim.Adam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9)), netD.get_optimizer()
    src, gt = (torch.from_numpy(syn.image(s, 1, 3, 32)).to(DEV) for s in (7, 8))
    totals, feats = [], []
    _clear()
    with DC.discriminator_conv_train("f16"):
        for _ in range(10):
            pred = torch.tanh(gen(src))
            l1 = F.l1_loss(pred, gt)
            out = adversarial_step(netD, opt_G, opt_D, {"L1": l1, "Total Loss": l1}, pred, gt)
            assert all(torch.isfinite(v).all() for v in out.values())
            totals.append((out["D_Fake"] + out["D_real"]).mean().item())
            feats.append(out["GAN_Feat"].item())
    print("discriminator totals:", " ".join(f"{t:.4f}" for t in totals))
    print("GAN_Feat:", " ".join(f"{t:.3f}" for t in feats))
    assert _flags()[0] == 0
    assert totals[-1] < totals[0]


def test_eval_and_no_grad_keep_the_parent_route(monkeypatch):
    """With isTrain false, or under no_grad, every convolution is the parent route's call -- F.conv2d with the same weight, stride and
    padding -- whatever the switch says: pinned by the calls themselves (ten F.conv2d per pass on bit-identical weights, none of the
    library's), and by the outputs' bits wherever two passes of the "torch" route give each other's bits (MIOpen's forward does not
    repeat its own from call to call on every stack, so a map behind such a layer has no bits to compare)."""
    fake = torch.from_numpy(syn.image(23, 1, 3, 32)).to(DEV)
    calls, real_call, convs, real_conv = [], _lib.call, [], F.conv2d
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real_call(name, *a, **k))[1])
    monkeypatch.setattr(F, "conv2d", lambda x, w, *a, **k: (convs.append((w.detach().clone(), a, k)), real_conv(x, w, *a, **k))[1])

    def passes(net, grad):
        out, seen = {}, {}
        with torch.enable_grad() if grad else torch.no_grad():
            for route in ("torch", "again", "f16"):
                del convs[:]
                with DC.discriminator_conv_train("f16" if route == "f16" else "torch"):
                    out[route] = [m for d in net(fake) for m in d]
                seen[route] = list(convs)
                assert [tuple(c[0].shape[:2]) for c in convs] == [(64, 3), (128, 64), (256, 128), (512, 256), (1, 512)] * 2
        for (w, a, k), (w2, a2, k2) in zip(seen["torch"], seen["f16"]):
            assert torch.equal(w, w2) and a == a2 and k == k2
        repeats = [torch.equal(a, b) for a, b in zip(out["torch"], out["again"])]
        same = [torch.equal(a, b) for a, b in zip(out["torch"], out["f16"])]
        print("the torch route repeats its bits:", repeats, "under the switch the same bits:", same)
        assert all(s for s, r in zip(same, repeats) if r)
        assert all("DiscConv" not in type(m.grad_fn).__name__ and "Lrelu" not in type(m.grad_fn).__name__ for m in out["f16"])

    passes(_net(64, isTrain=False).eval().to(DEV).netD.netD, True)       # isTrain false, grad mode on
    passes(_net(64).eval().to(DEV).netD.netD, False)                     # isTrain, no_grad
    assert not any(c.startswith("ps_disc_conv") for c in calls)
    assert DC.discriminator_conv_train.from_env({}) == "torch"          # and the default is the parent's route
