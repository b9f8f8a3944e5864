"""GPU: the backward pass of the split-fp16 3 x 3 convolution (csrc/conv_bwd.hip behind include/pixelsynth_conv_bwd.h, the autograd
Function networks/f16x3.py:conv3x3_train, the decoder blocks' opt-in decoder_conv_train).

Operator level: grad_input, grad_weight and grad_bias under the two assertions of tests/_conv_bwd_ref.py (its docstring says where they
come from) at three shapes and with gradients of 1e-7 .. 1e-10; exact results where the arithmetic leaves no choice (the halo, zeros,
a power-of-two factor on grad_y, two runs, the forward against the no-grad route).  Block level: a ResNet_Block in train() under the
opt-in against its fp64 twin with the same block in fp32 on the host as the yardstick, the default route untouched, ten Adam steps.
Every check prints its error / bound.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

import _conv_bwd_ref as ref
from pixelsynth_amd import _lib, synthetic as syn
from pixelsynth_amd.networks import architectures as A, f16x3

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
_REFS = {}


def _nhwc(t):
    return t.to(DEV).contiguous(memory_format=CL)


def _backward(x, w, b, g, needs=(True, True, True), grad_output=None):
    """conv3x3_train on the device and its backward pass -> (y, grad_x, grad_w, grad_bias), None where not asked for"""
    dx, dw = _nhwc(x).requires_grad_(needs[0]), w.to(DEV).requires_grad_(needs[1])
    db = None if b is None else b.to(DEV).requires_grad_(needs[2])
    y = f16x3.conv3x3_train(dx, dw, db)
    assert y.requires_grad and y.is_contiguous(memory_format=CL)
    y.backward(g.to(DEV) if grad_output is None else grad_output)
    torch.cuda.synchronize()
    return y.detach(), dx.grad, dw.grad, None if db is None else db.grad


def _reference(key, make):
    """The case's inputs and Reference, computed once and shared"""
    if key not in _REFS:
        x, w, b, g = make()
        _REFS[key] = (x, w, b, g, ref.reference(x, w, g))
    return _REFS[key]


def _check_case(name, x, w, b, g, r):
    _, gx, gw, gb = _backward(x, w, b, g)
    assert gx.shape == x.shape and gw.shape == w.shape and gb.shape == b.shape and gx.dtype == gw.dtype == gb.dtype == torch.float32
    assert gx.is_contiguous(memory_format=CL)
    ref.check(f"{name} grad_input", gx, r.x)
    ref.check(f"{name} grad_weight", gw, r.weight)
    ref.check(f"{name} grad_bias", gb, r.bias)
    return gx, gw, gb


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_three_gradients_against_fp64(shape):
    """Non-square frames with Ci != Co: a swapped axis or a wrong transpose is an error of the gradient's own size.  The second shape's
    reduction spans several parts with a partial last one, the third's is one part."""
    parts = ref.part_ranges(*shape)
    if shape == ref.SHAPES[1]:
        assert len(parts) > 1 and parts[-1][1] - parts[-1][0] < parts[0][1] - parts[0][0]
    if shape == ref.SHAPES[2]:
        assert len(parts) == 1
    assert len(parts) == _lib.call("ps_conv3x3_bwd_parts", *shape)
    x, w, b, g, r = _reference(shape, lambda: ref.inputs(*shape))
    assert r.s == 2.0 ** 12 or r.s == 2.0 ** 13
    f16x3.flag(DEV).zero_()
    _check_case("%d x %d x %d, %d -> %d" % shape, x, w, b, g, r)
    assert int(f16x3.flag(DEV).item()) == 0


def test_small_gradients_need_the_scaling():
    """g = 1e-7 * randn, one region 1e-10 * randn: without the power of two in front of the split the weight's gradient is off by 1e-1 of
    its size (tests/test_conv_bwd_cpu.py), fifty thousand times the bound"""
    shape = ref.SHAPES[0]
    x, w, b, g, r = _reference("small", lambda: ref.small_gradients(*shape))
    assert g.abs().max().item() < 1e-6 and r.s >= 2.0 ** 34
    _check_case("small gradients", x, w, b, g, r)


def test_a_power_of_two_on_grad_y_is_a_power_of_two_on_the_gradients():
    shape = ref.SHAPES[0]
    x, w, b, g, _ = _reference(shape, lambda: ref.inputs(*shape))
    _, gx, gw, gb = _backward(x, w, b, g)
    _, hx, hw, hb = _backward(x, w, b, g * 2.0 ** -9)
    assert torch.equal(hx, gx * 2.0 ** -9) and torch.equal(hw, gw * 2.0 ** -9) and torch.equal(hb, gb * 2.0 ** -9)


def test_two_runs_give_the_same_bits_and_the_forward_is_the_no_grad_route():
    shape = ref.SHAPES[1]
    x, w, b, g, _ = _reference(shape, lambda: ref.inputs(*shape))
    y1, gx1, gw1, gb1 = _backward(x, w, b, g)
    y2, gx2, gw2, gb2 = _backward(x, w, b, g)
    assert torch.equal(y1, y2) and torch.equal(gx1, gx2) and torch.equal(gw1, gw2) and torch.equal(gb1, gb2)
    with torch.no_grad():
        p = f16x3.pack3x3(w.to(DEV))
        y0 = f16x3.conv3x3(_nhwc(x), p, bias=b.to(DEV))
    assert torch.equal(y1, y0)


def test_only_what_requires_grad_gets_a_gradient():
    shape = ref.SHAPES[2]
    x, w, b, g, _ = _reference(shape, lambda: ref.inputs(*shape))
    _, gx, gw, gb = _backward(x, w, b, g)
    for needs in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        _, hx, hw, hb = _backward(x, w, b, g, needs)
        for full, got, need in ((gx, hx, needs[0]), (gw, hw, needs[1]), (gb, hb, needs[2])):
            assert (got is not None) == need and (not need or torch.equal(got, full)), needs
    _, hx, hw, hb = _backward(x, w, None, g)
    assert hb is None and torch.equal(hx, gx) and torch.equal(hw, gw)
    # a sliced grad_output (every other channel of a wider tensor, NCHW strides) is made channels-last-contiguous first
    wide = torch.zeros(g.size(0), 2 * g.size(1), g.size(2), g.size(3), device=DEV)
    wide[:, ::2] = g.to(DEV)
    sliced = wide[:, ::2]
    assert not sliced.is_contiguous() and not sliced.is_contiguous(memory_format=CL)
    _, hx, hw, hb = _backward(x, w, b, g, grad_output=sliced)
    assert torch.equal(hx, gx) and torch.equal(hw, gw) and torch.equal(hb, gb)
    # y.sum().backward(): grad_y is an expanded scalar
    dx, dw = _nhwc(x).requires_grad_(), w.to(DEV).requires_grad_()
    f16x3.conv3x3_train(dx, dw).sum().backward()
    _, ox, ow, _ = _backward(x, w, None, torch.ones_like(g))
    assert torch.equal(dx.grad, ox) and torch.equal(dw.grad, ow)


@pytest.mark.parametrize("pixel", [(0, 0), (0, 15), (31, 0), (31, 15), (13, 0)], ids=lambda p: "y%d_x%d" % p)
def test_the_halo_is_exact_zeros(pixel):
    """One non-zero pixel of g (two channels, one in each 32-channel tile) at a corner / on an edge of a 32 x 16 frame against x = 1 and a
    weight fp16 holds: every sum has at most two terms, all exact -- the gradients are T itself, and a tap that reads outside the frame
    is an exact 0 in grad_weight."""
    B, H, W, Ci, Co = 1, 32, 16, 64, 64
    gen = torch.Generator().manual_seed(3)
    x = torch.ones(B, Ci, H, W)
    w = torch.round(torch.randn(Co, Ci, 3, 3, generator=gen) * 0.1 * 256) / 256
    assert torch.equal(w, w.half().float())
    g = torch.zeros(B, Co, H, W)
    py, px = pixel
    g[0, 3, py, px], g[0, 40, py, px] = 0.75, -1.5
    r = ref.reference(x, w, g, has_bias=False)
    _, gx, gw, _ = _backward(x, w, None, g)
    assert torch.equal(gw.double().cpu(), r.weight.T) and torch.equal(gx.double().cpu(), r.x.T)
    assert torch.equal(r.weight.T, r.weight.g64) and torch.equal(r.x.T, r.x.g64)                # (T is the gradient: nothing was rounded)
    outside = 0
    for ky in range(3):
        for kx in range(3):
            inside = 0 <= py + ky - 1 < H and 0 <= px + kx - 1 < W
            outside += not inside
            for o, v in ((3, 0.75), (40, -1.5)):
                assert torch.equal(gw[o, :, ky, kx].cpu(), torch.full((Ci,), v if inside else 0.0)), (ky, kx, o)
    assert outside == (5 if pixel != (13, 0) else 3)
    assert not gw[[o for o in range(Co) if o not in (3, 40)]].any()


def test_zeros_and_values_that_are_not_finite():
    """g = 0: exact zeros.  One inf / one NaN in g: every output it reaches is not finite, the others are; the call returns, and the
    overflow flag of the forward -- which speaks of activations -- stays as it was."""
    shape = ref.SHAPES[0]
    B, H, W, Ci, Co = shape
    x, w, b, g, _ = _reference(shape, lambda: ref.inputs(*shape))
    _, gx, gw, gb = _backward(x, w, b, torch.zeros_like(g))
    assert not gx.any() and not gw.any() and not gb.any()
    f16x3.flag(DEV).zero_()
    for bad in (float("inf"), float("nan")):
        h = g.clone()
        h[1, 5, 9, 20] = bad
        _, gx, gw, gb = _backward(x, w, b, h)
        assert not torch.isfinite(gw[5]).any() and torch.isfinite(gw[[o for o in range(Co) if o != 5]]).all()
        assert not torch.isfinite(gb[5]) and torch.isfinite(gb[[o for o in range(Co) if o != 5]]).all()
        reach = torch.zeros(B, 1, H, W, dtype=torch.bool, device=DEV)
        reach[1, 0, 8:11, 19:22] = True
        assert not torch.isfinite(gx[reach.expand_as(gx)]).any() and torch.isfinite(gx[~reach.expand_as(gx)]).all()
        assert int(f16x3.flag(DEV).item()) == 0


# ---- the decoder's blocks -----------------------------------------------------------------------------------------------------------------------
def _block(seed=0):
    """ResNet_Block(64, 128), no resampling, with the generator's options (spectral norm), in train(): the convolutions' and the noise
    layers' weights train; the batch-norm statistics are the stored ones (the only form networks/architectures.py builds), randomised"""
    torch.manual_seed(seed)
    blk = A.ResNet_Block(64, 128, syn.network_opts())
    gen = torch.Generator().manual_seed(seed + 1)
    for m in blk.modules():
        if isinstance(m, A.bn):
            m.stored_mean.copy_(torch.randn(m.stored_mean.shape, generator=gen) * 0.2)
            m.stored_var.copy_(torch.rand(m.stored_var.shape, generator=gen) + 0.5)
    return _frozen_stats(blk.train())


def _frozen_stats(blk):
    for m in blk.modules():
        if isinstance(m, A.bn):
            m.eval()
    return blk


def _block_gradients(blk, x, noise, proj):
    """-> (y, {name: gradient}) of sum(blk(x) * proj), 'input' among the names"""
    x = x.clone().requires_grad_()
    y = blk(x, noise)
    (y * proj).sum().backward()
    grads = {n: p.grad for n, p in blk.named_parameters()}
    grads["input"] = x.grad
    return y.detach(), grads


def _spy(monkeypatch):
    calls, real = [], _lib.call

    def call(name, *args, **kw):
        calls.append(name)
        return real(name, *args, **kw)
    monkeypatch.setattr(_lib, "call", call)
    return calls


def _block_case():
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 64, 32, 32, generator=gen)
    noise = [torch.randn(2, A.NOISE_SZ, generator=gen) for _ in range(2)]
    proj = torch.randn(2, 128, 32, 32, generator=gen)
    return x, noise, proj


def test_a_decoder_block_trains_through_the_new_library(monkeypatch):
    cpu = _block()
    twin, dev = copy.deepcopy(cpu).double(), copy.deepcopy(cpu).to(DEV)
    x, noise, proj = _block_case()
    _, g64 = _block_gradients(twin, x.double(), [n.double() for n in noise], proj.double())
    _, g32 = _block_gradients(cpu, x, noise, proj)
    calls = _spy(monkeypatch)
    f16x3.flag(DEV).zero_()
    with f16x3.decoder_conv_train("f16x3"):
        _, got = _block_gradients(dev, _nhwc(x), [n.to(DEV) for n in noise], _nhwc(proj))
    torch.cuda.synchronize()
    assert calls.count("ps_conv3x3_grad_weight_f16x3") == 2 and calls.count("ps_conv3x3_bwd_prepare_f32") == 2     # both 3 x 3 layers
    assert calls.count("ps_conv3x3_bwd_unscale_f32") == 2 and calls.count("ps_conv3x3_f16x3_ex_nhwc") == 4         # forward and grad_input
    assert int(f16x3.flag(DEV).item()) == 0
    assert set(got) == set(g64) and {'input', 'ch_a.2.weight_orig', 'ch_a.5.weight_orig', 'ch_a.2.bias', 'ch_b.0.weight_orig'} <= set(got)
    for name in sorted(got):
        want = g64[name]
        E32 = (g32[name].double() - want).abs().max().item()
        err = (got[name].double().cpu() - want).abs().max().item()
        bound = 4 * max(E32, 1e-6 * want.abs().max().item())
        print(f"{name}: |g - g64| {err:.3e} <= {bound:.3e} ({err / bound:.3f} of the bound; E32 {E32:.3e}, max |g64| {want.abs().max().item():.3e})")
        assert got[name].shape == want.shape and err <= bound, name


def test_without_the_opt_in_nothing_changes(monkeypatch):
    """The default: output and gradients of a convolution in grad mode are torch's own, bit for bit, and the new library is not called"""
    monkeypatch.setattr(f16x3, "DECODER_CONV_TRAIN", "fp32")
    torch.manual_seed(2)
    conv = torch.nn.Conv2d(64, 128, 3, 1, 1).to(DEV).to(memory_format=CL)
    x, _, proj = _block_case()
    calls = _spy(monkeypatch)
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True       # (two calls of one MIOpen convolution: the same algorithm, no atomics)
    try:
        out = []
        for route in (lambda t: A._conv_split(conv, t)[0], lambda t: F.conv2d(t, conv.weight, conv.bias, 1, 1)):
            conv.zero_grad()
            xd = _nhwc(x).requires_grad_()
            y = route(xd)
            (y * _nhwc(proj)).sum().backward()
            out.append((y.detach(), xd.grad, conv.weight.grad.clone(), conv.bias.grad.clone()))
        # ... and a whole block in train() takes no entry point of the new library
        dev = copy.deepcopy(_block()).to(DEV)
        _block_gradients(dev, _nhwc(x), (None, None), _nhwc(proj))
    finally:
        torch.backends.cudnn.deterministic = was
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert not [c for c in calls if c in _lib.CONV_BWD_PROTOS or "f16x3" in c], calls


def test_ten_adam_steps_and_the_fast_path_sees_the_new_weights():
    dev = copy.deepcopy(_block(5)).to(DEV)
    x, noise, proj = _block_case()
    xd, nd, target = _nhwc(x), [n.to(DEV) for n in noise], _nhwc(proj) * 0.1
    conv = dev.ch_a[2]
    with torch.no_grad():
        a0 = torch.relu(xd)
        before = A._f16x3_conv(_frozen_stats(dev.eval()).ch_a[2], a0).clone()
    _frozen_stats(dev.train())
    opt = torch.optim.Adam(dev.parameters(), lr=2e-3)
    losses = []
    with f16x3.decoder_conv_train("f16x3"):
        for _ in range(10):
            opt.zero_grad()
            loss = (dev(xd, nd) - target).square().mean()
            loss.backward()
            opt.step()
            losses.append(loss.item())
    print("losses", " ".join(f"{v:.5f}" for v in losses))
    assert all(v == v for v in losses) and losses[-1] < losses[0]
    # the no-grad fast path packs the weight again (its cache is keyed by the weight's version) and is the Function's forward on it
    dev.eval()
    with torch.no_grad():
        fast = A._f16x3_conv(conv, a0)
        weight = A._plain_conv_weight(conv, a0)
        again = f16x3.conv3x3_train(a0, weight)
    assert fast is not None and torch.equal(fast, again) and not torch.equal(fast, before)
    f16x3.check_f16x3_overflow(DEV)
