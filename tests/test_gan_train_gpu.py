"""GPU: the discriminator's training kernels (csrc/gan_train.hip behind include/pixelsynth_gan_train.h, the autograd Functions of
networks/gan_train.py, MultiscaleDiscriminator and DiscriminatorLoss with opt.isTrain).

Operator level: instance norm + LeakyReLU forward and backward under the bounds of tests/_gan_train_ref.py (its docstring derives them)
at every form of the header's table and both sides of each boundary; an ill-conditioned plane, a NaN, two runs, a plane alone and in a
batch; the feature matching's values under its bound and its gradients bit for bit.  Network level: both steps against the fp64 twin
on the host, the two routes against each other, ten adversarial steps.  Every check prints its error / bound.
"""
import argparse
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _gan_train_ref as ref
from pixelsynth_amd import _lib, synthetic as syn
from pixelsynth_amd.losses import DiscriminatorLoss, adversarial_step
from pixelsynth_amd.networks import gan_train as GT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS, SLOPE = 1e-5, 0.2
# (N, C, H, W): the issue's shapes, then both sides of every boundary of the header's table -- 256 | 257 values (4 | 8 per lane of a
# wavefront), 2048 | 2049 (wavefront | workgroup; five planes: a last workgroup with one wavefront at work), 3072 | 3073 (12 | 16 per
# thread of a workgroup), 8192 | 8281 (resident | streaming)
CASES = [(1, 1, 1, 1), (2, 3, 1, 5), (3, 5, 7, 9), (2, 4, 8, 8), (2, 4, 65, 65), (1, 5, 16, 16), (1, 5, 1, 257), (1, 5, 32, 64), (1, 2, 3, 683),
         (1, 2, 48, 64), (1, 2, 7, 439), (1, 2, 64, 128), (1, 2, 91, 91)]
FORMS = {(1, 1, 1, 1): ("wave", 4), (2, 4, 65, 65): ("workgroup", 20), (1, 5, 16, 16): ("wave", 4), (1, 5, 1, 257): ("wave", 8),
         (1, 5, 32, 64): ("wave", 32), (1, 2, 3, 683): ("workgroup", 12), (1, 2, 48, 64): ("workgroup", 12), (1, 2, 7, 439): ("workgroup", 16),
         (1, 2, 64, 128): ("workgroup", 32), (1, 2, 91, 91): ("stream", 0)}


def _norm(x, dy=None):
    """The two entry points on the device -> y, mean, rstd (, dx)"""
    xd = x.to(DEV).contiguous()
    planes, hw = xd.size(0) * xd.size(1), xd.size(2) * xd.size(3)
    y = torch.empty_like(xd)
    mean, rstd = torch.empty(planes, device=DEV), torch.empty(planes, device=DEV)
    _lib.call("ps_in_lrelu_forward_f32", xd, planes, hw, EPS, SLOPE, y, mean, rstd, None, 0)
    out = [y, mean.view(xd.shape[:2]), rstd.view(xd.shape[:2])]
    if dy is not None:
        dx = torch.empty_like(xd)
        _lib.call("ps_in_lrelu_backward_f32", xd, dy.to(DEV).contiguous(), mean, rstd, planes, hw, SLOPE, dx, None, 0)
        out.append(dx)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def norm_against_fp64(shape, norm=_norm):
    """The body of test_norm_forward_and_backward_against_fp64 (tests/test_disc_routes_gpu.py runs its cases through it too, and gives a
    `norm` of its own: the entry points with their outputs inside rims)"""
    hw = shape[2] * shape[3]
    x, dy = ref.norm_inputs(shape, seed=sum(shape))
    y, mean, rstd, dx = norm(x, dy)
    f = ref.norm_forward64(x, EPS, SLOPE)
    mean_b, rstd_b, _ = ref.stat_bounds(f, EPS)
    assert ref.check("mean", mean, f["mean"], mean_b) <= 1.0
    assert ref.check("rstd", rstd, f["rstd"], rstd_b) <= 1.0
    assert ref.check("y", y, f["y"], ref.y_bound(x, f, EPS)) <= 1.0
    g64 = ref.norm_backward64(x, dy, EPS, SLOPE, y=y)
    bound, E32 = ref.grad_bound(ref.norm_autograd(x, dy, EPS, SLOPE, torch.float32), g64)
    assert ref.check("dx", dx, g64, bound) <= 1.0
    if hw == 1:
        assert not y.any() and not dx.any() and torch.equal(mean, x[:, :, 0, 0])
    # through the Function: the same bits, and it is the HIP route that ran
    xg = x.to(DEV).requires_grad_()
    out = GT.instance_norm_lrelu_train(xg, EPS, SLOPE)
    assert out.grad_fn is not None and type(out.grad_fn).__name__ == "_InLreluBackward"
    out.backward(dy.to(DEV))
    assert torch.equal(out.detach().cpu(), y) and torch.equal(xg.grad.cpu(), dx)
    with torch.no_grad():
        assert torch.equal(GT.instance_norm_lrelu_train(x.to(DEV), EPS, SLOPE).cpu(), y)


@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_norm_forward_and_backward_against_fp64(shape):
    hw = shape[2] * shape[3]
    assert FORMS.get(shape, ref.form(hw)) == ref.form(hw)
    norm_against_fp64(shape)


def test_an_ill_conditioned_plane():
    """100 + 0.01 randn: m2 = 1e4 over var = 1e-4.  The fp64 sums hold rstd; the fp32 m2 - mean^2 (its error is u m2 = 6e-4) does not"""
    gen = torch.Generator().manual_seed(5)
    for shape in ((2, 3, 33, 33), (1, 2, 65, 65), (1, 2, 91, 91)):
        x = 100 + 0.01 * torch.randn(*shape, generator=gen)
        y, mean, rstd = _norm(x)
        f = ref.norm_forward64(x, EPS, SLOPE)
        mean_b, rstd_b, _ = ref.stat_bounds(f, EPS)
        assert ref.check("mean", mean, f["mean"], mean_b) <= 1.0 and ref.check("rstd", rstd, f["rstd"], rstd_b) <= 1.0
        assert ref.check("y", y, f["y"], ref.y_bound(x, f, EPS)) <= 1.0
        m = x.mean((2, 3))
        naive = ((x * x).mean((2, 3)) - m * m).clamp_min(0).add(EPS).rsqrt()
        assert ref.check("rstd of the fp32 m2 - mean^2", naive, f["rstd"], rstd_b) > 1.0


@pytest.mark.parametrize("shape", [(2, 3, 17, 17), (1, 3, 65, 65), (1, 3, 91, 91)], ids=["wave", "workgroup", "stream"])
def test_planes_are_independent_and_runs_repeat(shape):
    x, dy = ref.norm_inputs(shape, seed=9)
    clean = _norm(x, dy)
    again = _norm(x, dy)
    assert all(torch.equal(a, b) for a, b in zip(clean, again))
    bad = x.clone()
    bad[0, 1, 3, 2] = float("nan")
    y, mean, rstd, dx = _norm(bad, dy)
    assert torch.isnan(y[0, 1]).all() and torch.isnan(dx[0, 1]).all() and torch.isnan(mean[0, 1]) and torch.isnan(rstd[0, 1])
    keep = torch.ones(shape[:2], dtype=torch.bool)
    keep[0, 1] = False
    for got, want in zip((y, mean, rstd, dx), clean):
        assert torch.equal(got[keep], want[keep])
    # a plane alone is the plane in its batch
    b, c = shape[0] - 1, 2
    alone = _norm(x[b:b + 1, c:c + 1].clone(), dy[b:b + 1, c:c + 1].clone())
    for got, want in zip(alone, clean):
        assert torch.equal(got[0, 0], want[b, c])


# ---------------------------------------------------------------- feature matching
MIXED = [(2, 1 + k % 3, 1 + 2 * k, 3 + k) for k in range(17)]
MAP_LISTS = {"one_value": [(2, 1, 1, 1)], "three": [(2, 3, 5, 7), (2, 8, 17, 17), (2, 1, 1, 1)], "three_pairs": [(6, 2, 3, 3)],
             "tile_plus_one": [(2, ref.TILE + 1)], "two_tiles_and_small": [(4, ref.TILE), (2, 5)], "sixteen": MIXED[:16], "seventeen": MIXED}


def _int_bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", list(MAP_LISTS))
def test_feature_matching_values_and_gradients(name):
    feature_matching_against_fp64(name, MAP_LISTS[name])


def feature_matching_against_fp64(name, shapes):
    """The body of test_feature_matching_values_and_gradients (tests/test_disc_routes_gpu.py runs its lists through it too) -> the
    maps, per_map and the total of the first run, on the host"""
    maps = ref.feat_maps(shapes, seed=len(shapes))
    w, gt = 5.0, 0.75
    leaves = [m.to(DEV).requires_grad_() for m in maps]
    calls, real = [], _lib.call
    _lib.call = lambda fn, *a, **k: (calls.append(fn), real(fn, *a, **k))[1]
    try:
        total, per_map = GT.feature_matching(leaves, w, per_map=True)
        total.backward(torch.tensor([gt], device=DEV))
    finally:
        _lib.call = real
    chunks = -(-len(shapes) // ref.MAX_MAPS)
    assert calls.count("ps_gan_feat_l1_f32") == calls.count("ps_gan_feat_l1_backward_f32") == chunks and total.shape == (1,)
    per64, tot64, mag = ref.feat_forward64(maps, [w] * len(maps))
    for k, m in enumerate(maps):
        n = m.numel() // 2
        assert abs(per_map[k].item() - per64[k]) <= ref.feat_value_bound(n, per64[k]), (k, per_map[k].item(), per64[k])
    n_all = sum(m.numel() // 2 for m in maps)
    bound = ref.feat_value_bound(n_all, mag) + (chunks - 1) * ref.U * abs(tot64)      # (two calls: one fp32 addition of their totals)
    print(f"{name}: total {total.item():.7g}, fp64 {tot64:.7g}, error / bound {abs(total.item() - tot64) / max(bound, 1e-300):.3f}")
    assert abs(total.item() - tot64) <= bound
    for leaf, want, m in zip(leaves, ref.feat_backward32(maps, [w] * len(maps), gt), maps):
        half = m.size(0) // 2
        got = leaf.grad.cpu()
        assert torch.equal(_int_bits(got), _int_bits(want))                           # bit for bit, the sign of every zero included
        assert not _int_bits(got[half:]).any()                                        # +0.0 in every real half
        assert not got[:half].reshape(-1)[::7].any() and got[:half].reshape(-1)[1::7].all()      # the planted ties, and nothing else
    # a map alone is the map among the others, and a second run is the first
    with torch.no_grad():
        t2, p2 = GT.feature_matching([m.to(DEV) for m in maps], w, per_map=True)
        assert torch.equal(t2, total.detach()) and torch.equal(p2, per_map)
        _, p_last = GT.feature_matching([maps[-1].to(DEV)], w, per_map=True)
        assert torch.equal(p_last[0], per_map[-1])
    return maps, per_map.cpu(), total.detach().cpu()


def test_feature_matching_keeps_a_nan_in_its_map():
    maps = ref.feat_maps(MAP_LISTS["three"], seed=4)
    dev = [m.to(DEV) for m in maps]
    _, clean = GT.feature_matching(dev, 5.0, per_map=True)
    dev[1][0, 2, 3, 4] = float("nan")
    leaves = [m.requires_grad_() for m in dev]
    total, per_map = GT.feature_matching(leaves, 5.0, per_map=True)
    total.backward()
    assert torch.isnan(per_map[1]) and torch.isnan(total).all() and torch.equal(per_map[[0, 2]], clean[[0, 2]])
    g = leaves[1].grad
    assert torch.isnan(g[0, 2, 3, 4]) and torch.isnan(g).sum() == 1 and not any(torch.isnan(l.grad).any() for l in (leaves[0], leaves[2]))


# ---------------------------------------------------------------- the whole network
def _opts(ndf, **kw):
    o = dict(discriminator_losses="pix2pixHD", gan_mode="hinge", norm_D="spectralinstance", ndf=ndf, output_nc=3, no_ganFeat_loss=False,
             isTrain=True, lambda_feat=10.0, lr=1e-3, niter=100, niter_decay=10)
    o.update(kw)
    return argparse.Namespace(**o)


def _net(ndf, seed=11):
    net = DiscriminatorLoss(_opts(ndf)).train()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in syn.fill_state_dict(shapes, seed).items()}, strict=True)
    return net


KINK = 2.0 ** -16
SEEDS = {8: (41, 42), 64: (47, 48)}    # ndf -> the seeds of the fake and the real images (test_the_network_against_its_fp64_twin)


def _both_steps(net, fake, real):
    """A generator step, then a discriminator step -> {name: tensor} of the losses, the gradient to the fake image and every parameter's
    gradient of both"""
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


@pytest.mark.parametrize("ndf,pairs,S", [(8, 2, 64), (64, 1, 32)], ids=["ndf8_2x64", "ndf64_1x32"])
def test_the_network_against_its_fp64_twin(ndf, pairs, S, monkeypatch):
    net = _net(ndf)
    twin64, twin32 = copy.deepcopy(net).double(), copy.deepcopy(net)
    fake, real = (torch.from_numpy(syn.image(s, pairs, 3, S)) for s in SEEDS[ndf])
    # The premise of comparing gradients: every LeakyReLU behind a norm has its branch decided.  The normalised value v is O(1), and an
    # fp32 network's v differs from the twin's by the rounding of the convolutions in front of it -- dot products of K = 2048 .. 8192
    # terms, about sqrt(K) u = 2^-18 each, over a few layers: KINK = 2^-16.  An element whose fp64 v is closer to 0 than that may take
    # either branch in ANY fp32 evaluation, and the other branch is a whole term (0.8 dy), not a rounding error.  The images (SEEDS) are
    # chosen so that the twin has no such element in either of its two passes (most seeds have a few among the 10^5 per pass; the smallest
    # |v| at these is 2e-5 and 4e-5), and the test holds them to it.
    undecided, formula = [], GT.norm_formula

    def spy(x, eps=1e-5, slope=0.2):
        undecided.append(int((ref.norm_forward64(x.detach(), eps, slope)["v"].abs() < KINK).sum()))
        return formula(x, eps, slope)
    monkeypatch.setattr(GT, "norm_formula", spy)
    want = _both_steps(twin64, fake.double(), real.double())
    monkeypatch.setattr(GT, "norm_formula", formula)
    assert len(undecided) == 12 and not any(undecided), undecided
    host32 = _both_steps(twin32, fake, real)
    calls, real_call = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real_call(name, *a, **k))[1])
    net = net.to(DEV)
    with GT.discriminator_train("hip"):
        got = _both_steps(net, fake.to(DEV), real.to(DEV))
    # six norms per forward, two forwards and two backwards; one feature-matching launch each way
    assert calls.count("ps_in_lrelu_forward_f32") == 12 and calls.count("ps_in_lrelu_backward_f32") == 12
    assert calls.count("ps_gan_feat_l1_f32") == 1 and calls.count("ps_gan_feat_l1_backward_f32") == 1
    assert set(got) == set(want) and len(got) == 7 + 2 * len(list(net.parameters()))
    worst = 0.0
    for k in want:
        bound, _ = ref.grad_bound(host32[k], want[k])
        worst = max(worst, ref.check(k, got[k], want[k], bound))
    print(f"ndf = {ndf}: largest error / bound {worst:.3f}")
    assert worst <= 1.0
    for k, v in net.state_dict().items():
        if k.endswith(("weight_u", "weight_v")):
            assert (v.cpu().double() - twin64.state_dict()[k]).abs().max() <= 1e-5, k


def test_the_routes_agree():
    fake, real = (torch.from_numpy(syn.image(s, 2, 3, 64)).to(DEV) for s in (23, 24))
    out = {}
    for route in ("hip", "torch"):
        # (weight seed 8: the hinge term GAN = -mean D(fake) is -0.18 on the host.  At seeds where it is a few 1e-3 it is the small
        # difference of outputs of either sign, and a relative error of it measures that cancellation, not the routes)
        net = _net(8, seed=8).to(DEV)
        with GT.discriminator_train(route):
            g = net.run_generator_one_step(fake, real)
            d = net.run_discriminator_one_step(fake, real)
        out[route] = {**{f"g/{k}": v for k, v in g.items()}, **{f"d/{k}": v for k, v in d.items()}}
    assert type(out["hip"]["g/GAN_Feat"].grad_fn).__name__ != type(out["torch"]["g/GAN_Feat"].grad_fn).__name__
    for k, v in out["hip"].items():
        w = out["torch"][k]
        print(k, v.item(), w.item())
        assert (v - w).abs().item() <= 1e-5 * w.abs().item(), k
    # the option selects the route like the switch
    net = DiscriminatorLoss(_opts(8, discriminator_train="torch")).train().to(DEV)
    assert "Lrelu" not in type(net.netD.netD.discriminator_0(fake)[1].grad_fn).__name__
    with GT.discriminator_train("hip"):
        assert type(net.netD.netD.discriminator_0(fake)[1].grad_fn).__name__ == "_InLreluBackward"


def test_ten_adversarial_steps_on_the_device():
    torch.manual_seed(0)
    netD = DiscriminatorLoss(_opts(8)).train().to(DEV)
    gen = nn.Conv2d(3, 3, 3, padding=1).to(DEV)
    opt_G, opt_D = torch.optim.Adam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9)), netD.get_optimizer()
    src, gt = (torch.from_numpy(syn.image(s, 2, 3, 64)).to(DEV) for s in (7, 8))
    totals, feats = [], []
    for _ in range(10):
        pred = torch.tanh(gen(src))
        l1 = F.l1_loss(pred, gt)
        out = adversarial_step(netD, opt_G, opt_D, {"L1": l1, "Total Loss": l1}, pred, gt)
        assert all(torch.isfinite(v).all() for v in out.values())
        totals.append((out["D_Fake"] + out["D_real"]).mean().item())
        feats.append(out["GAN_Feat"].item())
    print("discriminator totals:", " ".join(f"{t:.4f}" for t in totals))
    print("GAN_Feat:", " ".join(f"{t:.3f}" for t in feats))
    assert totals[-1] < totals[0]
