"""GPU: the training-mode batch norm (csrc/norm_train.hip behind include/pixelsynth_norm_train.h, the autograd Function
networks/norm_train.py:batch_norm_train, the decoder's blocks in train()).

Operator level: statistics, the update of the stored ones (bit for bit), y and the three gradients under the bounds of
tests/_norm_train_ref.py (its docstring derives them) at four shapes, with and without the ReLU, with per-sample and shared gain / bias;
the recomputed mask, an ill-conditioned channel, a NaN, two runs.  Block level: ResNet_Block(64, 128) fully in train() against its fp64
twin, the no-grad route with its pending bias, ten Adam steps of a small decoder.  Every check prints its error / bound.
"""
import copy

import pytest
import torch

import _norm_train_ref as ref
from pixelsynth_amd import _lib, synthetic as syn
from pixelsynth_amd.networks import architectures as A, f16x3, norm_train as NT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
EPS = 1e-5
CASES = [(3, 4, 20, 12), (2, 64, 32, 32), (1, 192, 16, 16), (2, 128, 48, 80)]
_REFS = {}
_WS = _lib.Workspace()


def _nhwc(t):
    return t.to(DEV).contiguous(memory_format=CL)


def _ops(x, gain, bias, dy=None, relu=True, pend=None, keep=0.9, mom=0.1, stored=None, want_dx=True):
    """The three entry points on the device -> dict of what they wrote (stored_mean / stored_var: the buffers after the update)"""
    B, C, H, W = x.shape
    xd = _nhwc(x)
    g, b = (t.expand(B, C).contiguous().to(DEV) for t in (gain, bias))
    sm, sv = (t.clone().to(DEV) for t in (stored or (torch.zeros(C), torch.ones(C))))
    mean, var, rstd = (torch.empty(C, device=DEV) for _ in range(3))
    ws = _WS.query(torch.device(DEV), "ps_norm_train_workspace_bytes", B, H * W, C)
    _lib.call("ps_norm_train_stats_f32", xd, None if pend is None else pend.to(DEV), B, H * W, C, EPS, keep, mom, sm, sv, mean, var, rstd,
              ws, ws.numel())
    y = torch.empty_like(xd)
    _lib.call("ps_norm_train_apply_f32", xd, mean, rstd, g, b, B, H * W, C, int(relu), y)
    out = dict(mean=mean, var=var, rstd=rstd, y=y, stored_mean=sm, stored_var=sv)
    if dy is not None:
        dx = torch.empty_like(xd) if want_dx else None
        dgain, dbias = torch.empty(B, C, device=DEV), torch.empty(B, C, device=DEV)
        _lib.call("ps_norm_train_backward_f32", xd, _nhwc(dy), mean, rstd, g, b, B, H * W, C, int(relu), dx, dgain, dbias, ws, ws.numel())
        out.update(dx=dx, dgain=dgain, dbias=dbias)
    torch.cuda.synchronize()
    return out


def _reference(shape, relu, shared):
    """The case's inputs, its fp64 forward, and the fp64 / fp32 host gradients -- computed once and shared"""
    key = (shape, relu, shared)
    if key not in _REFS:
        x, gain, bias, dy = ref.inputs(*shape, seed=sum(shape), shared=shared)
        B, C = shape[:2]
        f = ref.forward64(x, gain.expand(B, C), bias.expand(B, C), EPS, relu)
        flips = torch.zeros_like(dy, dtype=torch.bool)
        if relu:        # a mask that flips between fp32 and fp64 is not a rounding error: no gradient through the values next to 0
            flips = f["v"].abs() < 1e-4
            assert flips.float().mean().item() <= 0.01
            dy = torch.where(flips, torch.zeros_like(dy), dy)
        g64 = ref.autograd(x, gain, bias, dy, EPS, relu, torch.float64)
        g32 = ref.autograd(x, gain, bias, dy, EPS, relu, torch.float32)
        _REFS[key] = (x, gain, bias, dy, f, g64, g32, flips.float().mean().item())
    return _REFS[key]


@pytest.mark.parametrize("shared", [False, True], ids=["per_sample", "shared"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_statistics_output_and_gradients_against_fp64(shape, relu, shared):
    B, C, H, W = shape
    parts = ref.part_ranges(B, H * W)
    assert len(parts) == _lib.call("ps_norm_train_parts", B, H * W, C)
    if shape == CASES[3]:
        assert len(parts) > B and parts[-1][2] - parts[-1][1] < parts[0][2] - parts[0][1]        # several parts per frame, a partial last one
    x, gain, bias, dy, f, g64, g32, flipped = _reference(shape, relu, shared)
    name = "%dx%dx%dx%d %s %s" % (shape + ("relu" if relu else "linear", "shared" if shared else "per-sample"))
    gen = torch.Generator().manual_seed(1)
    stored = (torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5)
    pend = torch.randn(C, generator=gen)
    o = _ops(x, gain, bias, relu=relu, stored=stored, pend=pend)
    mean_b, var_b = ref.stat_bounds(x)
    assert ref.check(f"{name} mean", o["mean"], f["mean"], mean_b) <= 1.0
    assert ref.check(f"{name} var", o["var"], f["var"], var_b) <= 1.0
    assert torch.equal(o["rstd"].cpu(), (1.0 / torch.sqrt((o["var"].cpu() + EPS).double())).float())
    # the update: torch's fp32 expression on the kernel's own statistics, bit for bit -- with the pending bias, without, and standing
    mean, var = o["mean"].cpu(), o["var"].cpu()
    assert torch.equal(o["stored_mean"].cpu(), stored[0] * 0.9 + (mean + pend) * 0.1)
    assert torch.equal(o["stored_var"].cpu(), stored[1] * 0.9 + var * 0.1)
    o2 = _ops(x, gain, bias, relu=relu, stored=stored)
    assert torch.equal(o2["stored_mean"].cpu(), stored[0] * 0.9 + mean * 0.1) and torch.equal(o2["stored_var"].cpu(), stored[1] * 0.9 + var * 0.1)
    assert torch.equal(o2["mean"], o["mean"]) and torch.equal(o2["var"], o["var"]) and torch.equal(o2["y"], o["y"])     # (pend: the stored mean only)
    o3 = _ops(x, gain, bias, relu=relu, stored=stored, keep=1.0, mom=1.0)
    assert torch.equal(o3["stored_mean"].cpu(), stored[0] + mean) and torch.equal(o3["stored_var"].cpu(), stored[1] + var)
    assert ref.check(f"{name} y", o["y"], f["y"], ref.forward_bound(x, f)) <= 1.0
    assert o["y"].is_contiguous(memory_format=CL)
    # gradients through the autograd Function (a shared row's gradient is autograd's sum over the expansion)
    layer = A.bn(C).to(DEV).train()
    xd, gd, bd = _nhwc(x).requires_grad_(), gain.to(DEV).requires_grad_(), bias.to(DEV).requires_grad_()
    y = NT.batch_norm_train(xd, gd, bd, layer, relu)
    assert torch.equal(y.detach(), o["y"]) and y.requires_grad
    y.backward(_nhwc(dy))
    torch.cuda.synchronize()
    for what, got, w64, w32 in zip(("dx", "dgain", "dbias"), (xd.grad, gd.grad, bd.grad), g64, g32):
        bound, E32 = ref.grad_bound(w32, w64)
        r = ref.check(f"{name} {what} (E32 / max |g64| {E32 / w64.abs().max().item():.2e}, mask flips zeroed {flipped:.1e})", got, w64, bound)
        assert r <= 1.0, what


def test_the_recomputed_mask_is_the_forwards():
    shape = CASES[3]
    x, _, bias, _ = ref.inputs(*shape, seed=7)
    B, C = shape[:2]
    o = _ops(x, torch.ones(B, C), bias, dy=torch.ones(shape), relu=True)
    assert torch.equal(o["dbias"], (o["y"] > 0).sum((2, 3)).float()) and 0 < o["dbias"].min() and o["dbias"].max() < shape[2] * shape[3]


def test_an_ill_conditioned_channel_keeps_its_variance():
    shape = (2, 8, 16, 16)
    gen = torch.Generator().manual_seed(0)
    x = 100 + 0.01 * torch.randn(shape, generator=gen)
    gain, bias = 1 + 0.3 * torch.randn(2, 8, generator=gen), 0.3 * torch.randn(2, 8, generator=gen)
    m32 = x.mean((0, 2, 3))
    assert (((x * x).mean((0, 2, 3)) - m32 * m32) < 0).any()           # the fp32 formula loses it: rsqrt of that is a NaN
    x[:, 3] = 100.0                                                    # and one constant channel
    f = ref.forward64(x, gain, bias, EPS, True)
    o = _ops(x, gain, bias, relu=True)
    live = [c for c in range(8) if c != 3]
    mean_b, var_b = ref.stat_bounds(x)
    assert (o["var"][live] > 0).all() and ref.check("ill-conditioned var", o["var"], f["var"], var_b) <= 1.0
    assert ref.check("ill-conditioned mean", o["mean"], f["mean"], mean_b) <= 1.0
    assert 0 <= o["var"][3].item() <= 2.0 ** -40 * f["m2"][3].item()
    assert torch.isfinite(o["y"]).all() and ref.check("ill-conditioned y", o["y"][:, live], f["y"][:, live], ref.forward_bound(x, f)[:, live]) <= 1.0


def test_a_nan_stays_in_its_channel():
    shape = (2, 8, 16, 16)
    x, gain, bias, dy = ref.inputs(*shape, seed=9)
    clean = _ops(x, gain, bias, dy=dy, relu=True)
    bad = x.clone()
    bad[1, 5, 7, 3] = float("nan")
    o = _ops(bad, gain, bias, dy=dy, relu=True)
    others = [c for c in range(8) if c != 5]
    for k in ("mean", "var", "rstd", "stored_mean", "stored_var"):
        assert not torch.isfinite(o[k][5]) and torch.equal(o[k][others], clean[k][others]), k
    for k in ("y", "dx", "dgain", "dbias"):
        assert not torch.isfinite(o[k][:, 5]).any() and torch.equal(o[k][:, others], clean[k][:, others]), k
    assert all(torch.isfinite(clean[k]).all() for k in clean)


def test_two_runs_give_the_same_bits_and_dx_is_optional():
    shape = CASES[3]
    x, gain, bias, dy = ref.inputs(*shape, seed=11)
    a, b = _ops(x, gain, bias, dy=dy), _ops(x, gain, bias, dy=dy)
    assert all(torch.equal(a[k], b[k]) for k in a)
    c = _ops(x, gain, bias, dy=dy, want_dx=False)
    assert c["dx"] is None and torch.equal(c["dgain"], a["dgain"]) and torch.equal(c["dbias"], a["dbias"])
    # through the Function: no gradient for an input that needs none; it works under no_grad, where it saves nothing
    layer = A.bn(shape[1]).to(DEV).train()
    gd = gain.to(DEV).requires_grad_()
    y = NT.batch_norm_train(_nhwc(x), gd, bias.to(DEV), layer, True)
    y.backward(_nhwc(dy))
    assert torch.equal(gd.grad, a["dgain"]) and torch.equal(y.detach(), a["y"])
    with torch.no_grad():
        y0 = NT.batch_norm_train(_nhwc(x), gain.to(DEV), bias.to(DEV), layer, True)
    assert not y0.requires_grad and torch.equal(y0, a["y"])
    # what the kernels do not take goes the torch way: NCHW storage, fp64, C % 4 != 0
    xd = x.to(DEV)
    assert NT.takes(_nhwc(x)) and not NT.takes(xd) and not NT.takes(_nhwc(x).double()) and not NT.takes(_nhwc(x[:, :6]))
    y1 = NT.batch_norm_train(xd, gain.to(DEV), bias.to(DEV), layer, True)
    f = ref.forward64(x, gain, bias, EPS, True)
    assert ref.check("torch route y", y1, f["y"], 4 * ref.forward_bound(x, f) + 1e-6) <= 1.0


# ---- the decoder's blocks -----------------------------------------------------------------------------------------------------------------------
def _spy(monkeypatch):
    calls, real = [], _lib.call

    def call(name, *args, **kw):
        calls.append((name, args))
        return real(name, *args, **kw)
    monkeypatch.setattr(_lib, "call", call)
    return calls


def _count(calls, name):
    return sum(1 for n, _ in calls if n == name)


def _norms(blk):
    return [m for m in blk.modules() if isinstance(m, A.bn)]


def _block_gradients(blk, x, noise, proj):
    x = x.clone().requires_grad_()
    y = blk(x, noise)
    (y * proj).sum().backward()
    grads = {n: p.grad for n, p in blk.named_parameters()}
    grads["input"] = x.grad
    return y.detach(), grads


def _rule(name, got, want64, got32):
    bound, E32 = ref.grad_bound(got32, want64)
    r = ref.check(f"{name} (E32 {E32:.3e}, max |g64| {want64.abs().max().item():.3e})", got, want64, bound)
    assert r <= 1.0, name


def test_a_decoder_block_trains_on_batch_statistics(monkeypatch):
    """ResNet_Block(64, 128) fully in train(), nothing frozen, the convolutions on the fp16 matrix pipe: against its fp64 twin on the host,
    the same block in fp32 there as the yardstick"""
    torch.manual_seed(0)
    cpu = A.ResNet_Block(64, 128, syn.network_opts()).train()
    twin, dev, other = copy.deepcopy(cpu).double(), copy.deepcopy(cpu).to(DEV), copy.deepcopy(cpu).to(DEV)
    gen = torch.Generator().manual_seed(11)
    x = 0.3 + 1.5 * torch.randn(2, 64, 32, 32, generator=gen)
    noise = [torch.randn(2, A.NOISE_SZ, generator=gen) for _ in range(2)]
    proj = torch.randn(2, 128, 32, 32, generator=gen)
    y64, g64 = _block_gradients(twin, x.double(), [n.double() for n in noise], proj.double())
    y32, g32 = _block_gradients(cpu, x, noise, proj)
    calls = _spy(monkeypatch)
    f16x3.flag(DEV).zero_()
    with f16x3.decoder_conv_train("f16x3"):
        y, got = _block_gradients(dev, _nhwc(x), [n.to(DEV) for n in noise], _nhwc(proj))
    torch.cuda.synchronize()
    assert [_count(calls, "ps_norm_train_%s_f32" % k) for k in ("stats", "apply", "backward")] == [2, 2, 2]
    assert _count(calls, "ps_conv3x3_grad_weight_f16x3") == 2 and int(f16x3.flag(DEV).item()) == 0
    _rule("block output", y, y64, y32)
    assert set(got) == set(g64) and "input" in got and "ch_a.0.gain.weight_orig" in got
    for name in sorted(got):
        _rule(name, got[name], g64[name], g32[name])
    # the stored statistics: the first norm's inside the statistics' bounds (times the momentum, plus the update's three roundings),
    # the second's widened by the error of what is in front of it, four times that of the fp32 block on the host
    mean_b, var_b = ref.stat_bounds(x)
    for i, (d, t, c) in enumerate(zip(_norms(dev), _norms(twin), _norms(cpu))):
        for k, first in (("stored_mean", 0.1 * mean_b), ("stored_var", 0.1 * var_b)):
            want = getattr(t, k)
            E32 = (getattr(c, k).double() - want).abs().max().item()
            bound = 3 * ref.U * want.abs() + (first if i == 0 else 4 * max(E32, 1e-6 * want.abs().max().item()))
            assert ref.check(f"norm {i} {k} (E32 {E32:.3e})", getattr(d, k), want, bound) <= 1.0
    # under decoder_norm_train("torch") no entry point of the library is called
    del calls[:]
    with NT.decoder_norm_train("torch"), f16x3.decoder_conv_train("f16x3"):
        _block_gradients(other, _nhwc(x), [n.to(DEV) for n in noise], _nhwc(proj))
    assert not [n for n, _ in calls if n in _lib.NORM_TRAIN_PROTOS] and _count(calls, "ps_conv3x3_grad_weight_f16x3") == 2


@pytest.mark.parametrize("widths,kind", [((8, 16), "Down"), ((16, 8), "Up")], ids=["down", "up"])
def test_the_no_grad_route_with_its_pending_bias(widths, kind, monkeypatch):
    """train() under no_grad -- how standing statistics are collected: the first convolution's bias is still missing from what the second
    norm reads and goes in as `pend`.  Output and stored statistics against the grad-mode route's, each against the fp64 twin"""
    torch.manual_seed(4)
    cpu = A.ResNet_Block(widths[0], widths[1], syn.network_opts(), kind).train()
    twin, a, b = copy.deepcopy(cpu).double(), copy.deepcopy(cpu).to(DEV), copy.deepcopy(cpu).to(DEV)
    gen = torch.Generator().manual_seed(5)
    x = 0.3 + 1.5 * torch.randn(2, widths[0], 16, 16, generator=gen)
    noise = [torch.randn(2, A.NOISE_SZ, generator=gen) for _ in range(2)]
    y64 = twin(x.double(), [n.double() for n in noise]).detach()
    y32 = cpu(x, noise).detach()
    calls = _spy(monkeypatch)
    ya = a(_nhwc(x).requires_grad_(), [n.to(DEV) for n in noise]).detach()
    pends = [args[1] is not None for n, args in calls if n == "ps_norm_train_stats_f32"]
    assert pends == [False, False]
    del calls[:]
    with torch.no_grad():
        yb = b(_nhwc(x), [n.to(DEV) for n in noise])
    pends = [args[1] is not None for n, args in calls if n == "ps_norm_train_stats_f32"]
    assert pends == [False, True] and _count(calls, "ps_norm_train_apply_f32") == 2
    _rule(f"{kind} grad-mode output", ya, y64, y32)
    _rule(f"{kind} no-grad output", yb, y64, y32)
    for i, (na, nb, t, c) in enumerate(zip(_norms(a), _norms(b), _norms(twin), _norms(cpu))):
        for k in ("stored_mean", "stored_var"):
            _rule(f"{kind} norm {i} {k}, grad mode", getattr(na, k), getattr(t, k), getattr(c, k))
            _rule(f"{kind} norm {i} {k}, no grad", getattr(nb, k), getattr(t, k), getattr(c, k))


def test_a_small_decoder_takes_ten_adam_steps(monkeypatch):
    torch.manual_seed(6)
    dec = A.get_decoder(syn.network_opts(ngf=8)).to(DEV).train()
    norms = _norms(dec)
    assert len(norms) == 16 and [m.stored_mean.numel() for m in norms][-1] == 3
    before = [(m.stored_mean.clone(), m.stored_var.clone()) for m in norms]
    gen = torch.Generator().manual_seed(7)
    x = torch.rand(2, 3, 32, 32, generator=gen).to(DEV) * 2 - 1
    mask = (torch.rand(2, 32, 32, generator=gen) < 0.2).to(DEV)
    target = torch.rand(2, 3, 32, 32, generator=gen).to(DEV) * 2 - 1
    noise = [torch.randn(2, A.NOISE_SZ, generator=gen).to(DEV) for _ in range(dec.n_noise())]
    calls = _spy(monkeypatch)
    opt = torch.optim.Adam(dec.parameters(), lr=2e-3)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = (dec(x, mask, noise) - target).square().mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("losses", " ".join(f"{v:.5f}" for v in losses))
    assert all(v == v and abs(v) != float("inf") for v in losses) and losses[-1] < losses[0]
    # every norm but the last (C = 3: the torch route) went through the library, and every one has moved
    assert [_count(calls, "ps_norm_train_%s_f32" % k) for k in ("stats", "apply", "backward")] == [150, 150, 150]
    for m, (m0, v0) in zip(norms, before):
        assert not torch.equal(m.stored_mean, m0) and not torch.equal(m.stored_var, v0) and torch.isfinite(m.stored_mean).all()
    # eval() afterwards: the existing fast path, on the new statistics
    del calls[:]
    dec.eval()
    with torch.no_grad():
        out = dec(x, mask, noise)
    names = [n for n, _ in calls]
    assert "ps_noise_affine_f32" in names and not [n for n in names if n in _lib.NORM_TRAIN_PROTOS]
    assert out.shape == (2, 3, 32, 32) and torch.isfinite(out).all()
    f16x3.check_f16x3_overflow(DEV)
