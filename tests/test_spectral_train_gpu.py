"""GPU: the batched spectral normalisation (csrc/spectral_train.hip through networks/spectral_train.py) against the fp64 mirror of
tests/_spectral_ref.py on the same fp32 inputs, under its bounds: forward values iterating and not, the gradient, the in-place
semantics, the bits, the launch count, the three networks against their fp64 twins and the torch route, ten Adam steps."""
import copy
import re

import pytest
import torch
import torch.nn as nn
from torch.nn.utils.spectral_norm import SpectralNorm

import _spectral_ref as ref
from _forward_train_util import train_opts
from pixelsynth_amd import _lib
from pixelsynth_amd.networks import architectures as arch, discriminators as D, routing, spectral_train as ST

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = ref.SHAPES + ref.BOUNDARY_SHAPES


def make_layer(R, C, iterate, seed=0, conv=None):
    """A spectral-normalised Linear (R, C) on the GPU with ref.layer_inputs' values -- or, conv = (Ci, k), a Conv2d whose weight lies in
    channels-last storage, as the networks' do -- in train(iterate); -> (module, W, u, v) with the fp32 inputs on the host, W as (R, C)"""
    W, u, v = ref.layer_inputs(R, C, seed)
    if conv:
        mod = nn.utils.spectral_norm(nn.Conv2d(conv[0], R, conv[1]))
        assert mod.weight_orig[0].numel() == C
    else:
        mod = nn.utils.spectral_norm(nn.Linear(C, R, bias=False))
    with torch.no_grad():
        mod.weight_orig.copy_(W.view_as(mod.weight_orig)), mod.weight_u.copy_(u), mod.weight_v.copy_(v)
    mod = mod.to(DEV).train(iterate)
    if conv:
        mod = mod.to(memory_format=torch.channels_last)
        assert ST._interleave(mod.weight_orig) == conv[0]
    return mod, W, u, v


def run(layers):
    """normalise() on the modules of `layers` in one call -> the pending weights, taken"""
    mods = [layer[0] for layer in layers]
    assert ST.normalise(mods) == mods
    return [routing.take_pending(m) for m in mods]


def forward_ratios(layer, w, iterate, tag):
    """The largest error / bound of v, u, sigma (through W_sn) and W_sn of one layer; a layer that does not iterate keeps u and v's bits"""
    mod, W, u, v = layer
    f, h = ref.forward64(W, u, v, iterate), ref.hook32(W, u, v, iterate)
    e = ref.forward_errors(W, u, v, iterate, f)
    R = W.size(0)
    got = dict(v=mod.weight_v, u=mod.weight_u, w=w.detach().reshape(R, -1))
    if not iterate:
        assert torch.equal(mod.weight_u.cpu(), u) and torch.equal(mod.weight_v.cpu(), v)
    # sigma as the kernel stored it shows in W_sn alone; W / W_sn at W's largest entry recovers it to two roundings, inside its bound's U
    worst = max(ref.check(f"{tag} {k}", got[k], f[k], ref.bounded(e[k], h[k], f[k])) for k in ("v", "u", "w"))
    at = W.abs().argmax()
    sigma = W.reshape(-1)[at].double() / got["w"].reshape(-1)[at].double().cpu()
    bound = ref.bounded(e["sigma"] + 2 * ref.U * f["sigma"].abs(), h["sigma"], f["sigma"])
    return max(worst, ref.check(f"{tag} sigma", sigma, f["sigma"], bound))


@pytest.fixture(scope="module")
def tables():
    """Both tables (iterating, not iterating) of all shapes, run once: (layers, weights, copies of u and v after the pass)"""
    out = {}
    for iterate in (True, False):
        layers = [make_layer(R, C, iterate) for R, C in ALL]
        ws = run(layers)
        out[iterate] = (layers, ws, [(m.weight_u.clone(), m.weight_v.clone()) for m, *_ in layers])
    return out


@pytest.mark.parametrize("iterate", [True, False])
def test_forward_values_of_the_table(tables, iterate):
    layers, ws, _ = tables[iterate]
    worst = max(forward_ratios(layer, w, iterate, f"table {R}x{C}") for layer, w, (R, C) in zip(layers, ws, ALL))
    print("largest error / bound:", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("iterate", [True, False])
@pytest.mark.parametrize("shape", ALL, ids=lambda s: "%dx%d" % s)
def test_a_layer_alone_has_the_tables_values_and_bits(tables, shape, iterate):
    layer = make_layer(*shape, iterate)
    (w,) = run([layer])
    assert forward_ratios(layer, w, iterate, "alone %dx%d" % shape) <= 1.0
    k = ALL.index(shape)
    _, ws, uv = tables[iterate]
    assert torch.equal(w, ws[k]) and torch.equal(layer[0].weight_u, uv[k][0]) and torch.equal(layer[0].weight_v, uv[k][1])


@pytest.mark.parametrize("iterate", [True, False])
def test_a_channels_last_convolution_weight(iterate):
    """What the networks hand over on the GPU: (Co, Ci, kh, kw) in channels-last storage; u and v belong to the (Co, Ci kh kw) matrix"""
    for R, Ci, k in ((5, 6, 3), (8, 3, 4), (130, 12, 3)):
        layer = make_layer(R, Ci * k * k, iterate, conv=(Ci, k))
        (w,) = run([layer])
        assert w.shape == layer[0].weight_orig.shape and w.stride() == layer[0].weight_orig.stride()
        assert forward_ratios(layer, w, iterate, f"conv {R}x{Ci}x{k}x{k}") <= 1.0
        G = torch.randn(w.shape, generator=torch.Generator().manual_seed(R)).to(DEV)        # (contiguous: copied into the weight's layout)
        w.backward(G)
        f = ref.forward64(layer[1], layer[2], layer[3], iterate)
        dW = ref.backward64(f, G)
        bound = ref.bounded(ref.backward_error(f, ref.forward_errors(layer[1], layer[2], layer[3], iterate, f), G, dW),
                            ref.autograd(layer[1], layer[2], layer[3], iterate, G, torch.float32), dW)
        grad = layer[0].weight_orig.grad
        assert grad.stride() == w.stride() and ref.check(f"conv {R}x{Ci}x{k}x{k} dW", grad.reshape(R, -1), dW, bound) <= 1.0


def grads_of(kind, ws, skip):
    """G per layer: randn, or W_sn + 0.1 randn (then d is large); None for the layers of `skip`"""
    out = []
    for k, w in enumerate(ws):
        g = torch.randn(w.shape, generator=torch.Generator().manual_seed(100 + k)).to(DEV)
        out.append(None if k in skip else g if kind == "randn" else w.detach() + 0.1 * g)
    return out


@pytest.mark.parametrize("iterate", [True, False])
@pytest.mark.parametrize("kind", ["randn", "correlated"])
def test_the_gradient_against_fp64_autograd(kind, iterate):
    layers = [make_layer(R, C, iterate) for R, C in ALL]
    ws = run(layers)
    skip = {1, 6, len(ALL) - 1}
    Gs = grads_of(kind, ws, skip)
    torch.autograd.backward([w for w, g in zip(ws, Gs) if g is not None], [g for g in Gs if g is not None])
    worst = 0.0
    for k, ((mod, W, u, v), G, (R, C)) in enumerate(zip(layers, Gs, ALL)):
        grad = mod.weight_orig.grad
        if G is None:           # a gradient of zeros
            assert grad is not None and grad.shape == (R, C) and not grad.any()
            continue
        f = ref.forward64(W, u, v, iterate)
        dW = ref.backward64(f, G)
        assert (dW - ref.autograd(W, u, v, iterate, G, torch.float64)).abs().max() <= 1e-12 * dW.abs().max()
        bound = ref.bounded(ref.backward_error(f, ref.forward_errors(W, u, v, iterate, f), G, dW),
                            ref.autograd(W, u, v, iterate, G, torch.float32), dW)
        worst = max(worst, ref.check(f"{R}x{C} dW {kind}", grad, dW, bound))
        if kind == "correlated" and R * C > 1:      # this G is what a backward without the u v^T term would miss by far
            assert ref.check(f"{R}x{C} dW without u v^T", G.double().cpu() / f["sigma"], dW, bound) > 10.0
    print("largest error / bound:", worst)
    assert worst <= 1.0


def test_the_backward_reads_the_vectors_of_its_own_forward():
    mod, W, u, v = make_layer(130, 300, True)
    (w1,) = run([(mod, W, u, v)])
    u1, v1 = mod.weight_u.cpu().clone(), mod.weight_v.cpu().clone()
    assert not torch.equal(u1, u) and not torch.equal(v1, v)                          # an iterating layer updates its vectors
    (w2,) = run([(mod, W, u, v)])
    assert not torch.equal(mod.weight_u.cpu(), u1) and not torch.equal(w1, w2)        # ... at every forward
    G = w1.detach() + 0.1 * torch.randn_like(w1)
    w1.backward(G)
    f = ref.forward64(W, u, v, True)                    # the first forward's
    dW = ref.backward64(f, G)
    bound = ref.bounded(ref.backward_error(f, ref.forward_errors(W, u, v, True, f), G, dW), ref.autograd(W, u, v, True, G, torch.float32), dW)
    assert ref.check("the first forward's dW", mod.weight_orig.grad, dW, bound) <= 1.0
    second = ref.backward64(ref.forward64(W, u1, v1, True), G)
    assert ref.check("the second forward's dW", mod.weight_orig.grad, second, bound) > 1.0
    # the version counters move as the hook's copy_ moves them; a layer that does not iterate leaves its vectors' bits and versions
    still, W, u, v = make_layer(130, 300, False)
    before = (still.weight_u._version, still.weight_v._version)
    run([(still, W, u, v)])
    assert torch.equal(still.weight_u.cpu(), u) and torch.equal(still.weight_v.cpu(), v)
    assert (still.weight_u._version, still.weight_v._version) == before
    before = (mod.weight_u._version, mod.weight_v._version)
    run([(mod, W, u, v)])
    assert mod.weight_u._version > before[0] and mod.weight_v._version > before[1]
    # without grad mode: forward only
    with torch.no_grad():
        (w3,) = run([(mod, W, u, v)])
    assert not w3.requires_grad and w2.requires_grad


def test_twice_gives_the_same_bits_and_nan_stays():
    def once():
        layers = [make_layer(R, C, True) for R, C in ALL]
        ws = run(layers)
        Gs = grads_of("correlated", ws, {2})
        torch.autograd.backward([w for w, g in zip(ws, Gs) if g is not None], [g for g in Gs if g is not None])
        return [t for (m, *_), w in zip(layers, ws) for t in (w.detach(), m.weight_u, m.weight_v, m.weight_orig.grad)]
    a, b = once(), once()
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    # a zero matrix: sigma = 0, a weight of NaN, as torch's; its neighbours in the table are untouched
    zero, *_ = make_layer(5, 7, True)
    with torch.no_grad():
        zero.weight_orig.zero_()
    planted, W, u, v = make_layer(16, 64, True)
    with torch.no_grad():
        planted.weight_orig[3, 5] = float("nan")
    clean = make_layer(64, 20, True)
    wz, wp, wc = run([(zero,), (planted,), clean])
    assert torch.isnan(wz).all() and not zero.weight_u.any() and not zero.weight_v.any()
    h = ref.hook32(torch.zeros(5, 7), *ref.layer_inputs(5, 7)[1:], True)
    assert torch.isnan(h["w"]).all() and not h["u"].any()
    assert torch.isnan(wp[3, 5]) and torch.isnan(wp).all() and torch.isnan(planted.weight_u).all()   # (it reaches sigma, as in torch)
    assert forward_ratios(clean, wc, True, "beside NaN") <= 1.0


def sn_kernels(fn):
    """Names of the k_sn_* kernels fn() runs, by torch's profiler"""
    from torch.profiler import ProfilerActivity, profile
    fn()                                            # (tables, workspaces)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sorted(re.search(r"k_sn_[a-z]+", ev.name).group(0) for ev in prof.events()
                  if ev.device_type == torch.autograd.DeviceType.CUDA and "k_sn_" in ev.name)


def decoder(seed=0):
    torch.manual_seed(seed)
    return arch.get_decoder(train_opts()).to(DEV).train()


def test_the_launch_count_does_not_depend_on_the_layers():
    def step(mods):
        def fn():
            taken = ST.normalise(mods)
            assert len(taken) == len(mods)
            ws = [routing.take_pending(m) for m in mods]
            torch.autograd.backward(ws, [torch.ones_like(w) for w in ws])
        return fn
    one = sn_kernels(step([make_layer(64, 20, True)[0]]))
    mods = ST.sn_modules(decoder())
    many = sn_kernels(step(mods))
    assert len(mods) == 54
    assert one == many == sorted(["k_sn_wtu", "k_sn_v", "k_sn_wv", "k_sn_u", "k_sn_div", "k_sn_dot", "k_sn_dw"])
    assert len(one) == ref.FORWARD_LAUNCHES + ref.BACKWARD_LAUNCHES


# ---- the three networks at small sizes -----------------------------------------------------------------------------------------------

def _unet():
    torch.manual_seed(2)
    return arch.Unet(num_filters=4, channels_in=3, channels_out=1, opt=train_opts()).to(DEV).train()


def _disc():
    torch.manual_seed(3)
    return D.define_D(train_opts()).to(DEV).train()


def _inputs(name):
    gen = torch.Generator().manual_seed(7)
    if name == "decoder":
        return (torch.randn(1, 3, 16, 16, generator=gen), torch.rand(1, 16, 16, generator=gen) > 0.5,
                [torch.randn(1, arch.NOISE_SZ, generator=gen) for _ in range(16)])
    if name == "unet":
        return (torch.randn(1, 3, 256, 256, generator=gen),)
    return (torch.randn(1, 3, 32, 32, generator=gen),)


NETWORKS = {"decoder": (decoder, 54), "unet": (_unet, 16), "discriminator": (_disc, 6)}


def _loss(out):
    maps = [m for scale in out for m in scale] if isinstance(out, list) else [out]
    return sum(m.square().mean() for m in maps), torch.cat([m.reshape(-1) for m in maps])


def _to(args, device, dtype=None):
    conv = lambda t: t.to(device, dtype if t.is_floating_point() else None)
    return tuple([conv(x) for x in a] if isinstance(a, list) else conv(a) for a in args)


def _run(net, args):
    net.zero_grad()
    out = net(*args)
    loss, flat = _loss(out)
    loss.backward()
    return flat.detach(), {k: p.grad for k, p in net.named_parameters() if k.endswith("weight_orig")}


@pytest.mark.parametrize("name", list(NETWORKS))
def test_the_networks_against_their_fp64_twins_and_the_torch_route(name, monkeypatch):
    """The small networks under "hip" against their fp64 twins on the host, under the gradient rule 4 max(E32, 1e-6 max |fp64|), E32 the
    fp32 twin's own error on the host; the spies; the stored vectors under the forward bounds.

    Measured on the MI355X: outputs at 0.18 (decoder), 0.24 (Unet), 0.19 (discriminator) of the rule; every weight_orig gradient of the
    decoder at most 0.31, of the Unet 0.60, of the discriminator 0.23.  (While the kernels still rounded t, |t|, s and |s| to fp32 the
    decoder case missed the rule on one of its 54 gradients, eblocks.0.ch_a.0.gain.weight_orig, at 1.087; it is now at 0.12.)"""
    make, n_sn = NETWORKS[name]
    hooks, calls = [], []
    real_hook, real_call = SpectralNorm.compute_weight, _lib.call
    monkeypatch.setattr(SpectralNorm, "compute_weight",
                        lambda self, m, do_power_iteration: (hooks.append(1), real_hook(self, m, do_power_iteration))[1])
    monkeypatch.setattr(_lib, "call", lambda fn, *a, **k: (calls.append(fn), real_call(fn, *a, **k))[1])
    monkeypatch.setattr(torch.backends.cudnn, "enabled", False)         # the library convolutions repeat their bits
    args = _inputs(name)
    net = make()
    start = copy.deepcopy(net.state_dict())
    twin64, twin32 = copy.deepcopy(net).cpu().double(), copy.deepcopy(net).cpu()
    y64, g64 = _run(twin64, _to(args, "cpu", torch.float64))
    del hooks[:]
    y32, g32 = _run(twin32, _to(args, "cpu", torch.float32))
    hook_calls_host = len(hooks)
    # the default: the hook, called exactly as before (the discriminator's _SNConv restates it and never calls it)
    del hooks[:], calls[:]
    y_t, g_t = _run(net, _to(args, DEV))
    assert len(hooks) == hook_calls_host == (0 if name == "discriminator" else n_sn) and not [c for c in calls if "spectral" in c]
    uv_t = [k for k in net.state_dict() if k.endswith(("weight_u", "weight_v"))]
    net.load_state_dict(start)
    del hooks[:], calls[:]
    with ST.spectral_train("hip"):
        y_h, g_h = _run(net, _to(args, DEV))
    assert not hooks and calls.count("ps_spectral_forward_f32") == 1 and calls.count("ps_spectral_backward_f32") == 1
    assert not any(routing.has_pending(m) for m in net.modules())
    rule = lambda a32, a64: 4 * max((a32.double() - a64).abs().max().item(), 1e-6 * a64.abs().max().item())
    assert ref.check(f"{name} output", y_h, y64, rule(y32, y64)) <= 1.0
    assert len(g_h) == n_sn == len(g64)
    for k in g64:               # (the torch route on the same device under the same rule: printed, not asserted)
        ref.check(f"{name} {k} (torch route)", g_t[k], g64[k], rule(g32[k], g64[k]))
    worst = max(ref.check(f"{name} {k}", g_h[k], g64[k], rule(g32[k], g64[k])) for k in g64)
    print("largest gradient error / bound:", worst)
    assert worst <= 1.0
    # the stored vectors after the forward: within the forward bounds of the torch route's
    mods = dict(net.named_modules())
    for key in uv_t:
        prefix, which = key.rsplit(".", 1)
        W = start[prefix + ".weight_orig"].cpu()
        u, v = start[prefix + ".weight_u"].cpu(), start[prefix + ".weight_v"].cpu()
        f, h = ref.forward64(W, u, v, True), ref.hook32(W, u, v, True)
        k = which[-1]
        bound = ref.bounded(ref.forward_errors(W, u, v, True, f)[k], h[k], f[k])
        assert ref.check(f"{name} {key}", mods[prefix].state_dict()[which], f[k], bound) <= 1.0


def test_ten_adam_steps_of_the_small_decoder():
    net = decoder(5)
    x, mask, noise = _to(_inputs("decoder"), DEV)
    target = torch.tanh(torch.randn(1, 3, 16, 16, generator=torch.Generator().manual_seed(9))).to(DEV)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.0, 0.9))
    losses = []
    with ST.spectral_train("hip"):
        for _ in range(10):
            opt.zero_grad()
            loss = (net(x, mask, noise) - target).abs().mean()
            loss.backward()
            assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)
            opt.step()
            losses.append(loss.item())
    print("losses:", " ".join(f"{v:.4f}" for v in losses))
    assert losses[-1] < losses[0] and all(torch.isfinite(p).all() for p in net.parameters())
