"""GPU: what a decoder block trains through between its convolutions and its norms (csrc/block_train.hip behind
include/pixelsynth_block_train.h, the autograd Functions of networks/block_train.py, the blocks' opt-in decoder_block_train).

Operator level: the two resampling adjoints and the three gradients of the 1 x 1 convolution under the bounds of tests/_block_train_ref.py
(its docstring derives them), exact results where the arithmetic leaves no choice (one-hot gradients, zeros, two runs, the forward passes
against the no-grad kernels).  Block level: a Down and an Up ResNet_Block in train() under all the opt-ins against their fp64 twins with
the same block in fp32 on the host as the yardstick, the default route untouched, ten Adam steps.  Every check prints its error / bound.
"""
import copy

import pytest
import torch

import _block_train_ref as ref
from pixelsynth_amd import _lib, synthetic as syn
from pixelsynth_amd.networks import architectures as A, block_train as BT, f16x3

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
_REFS = {}


def _nhwc(t):
    return t.to(DEV).contiguous(memory_format=CL)


def _rule(name, got, want64, got32):
    bound, E32 = ref.grad_bound(got32, want64)
    r = ref.check(f"{name} (E32 {E32:.3e}, max |g64| {want64.abs().max().item():.3e})", got, want64, bound)
    assert r <= 1.0, name
    return r


# ---- the adjoints ---------------------------------------------------------------------------------------------------------------------------
def _adjoint(kind, g, shape, b=True):
    """resample_sum_train's backward pass on g -> (gradient of a, gradient of b or None)"""
    a = torch.zeros(shape, device=DEV).contiguous(memory_format=CL).requires_grad_()
    b = torch.zeros(shape, device=DEV).contiguous(memory_format=CL).requires_grad_() if b else None
    out = BT.resample_sum_train(kind, a, b)
    assert out.requires_grad and out.is_contiguous(memory_format=CL) and out.shape == g.shape
    out.backward(_nhwc(g))
    torch.cuda.synchronize()
    return a.grad, None if b is None else b.grad


def _adjoint_case(kind, shape4):
    key = (kind,) + shape4
    if key not in _REFS:
        B, H, W, C = shape4
        shape = (B, C, H, W)
        gen = torch.Generator().manual_seed(sum(shape4))
        g = torch.randn(ref.resample(kind, torch.zeros(shape)).shape, generator=gen)
        _REFS[key] = (shape, g, ref.adjoint(kind, g, shape), ref.adjoint(kind, g, shape, torch.float32), ref.adjoint_bound(kind, g, shape))
    return _REFS[key]


@pytest.mark.parametrize("kind,shape4", [("Up", s) for s in ref.UP_SHAPES] + [("Down", s) for s in ref.DOWN_SHAPES],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_the_adjoints_against_fp64(kind, shape4):
    shape, g, y64, y32, bound = _adjoint_case(kind, shape4)
    ga, gb = _adjoint(kind, g, shape)
    assert ga.shape == shape and ga.is_contiguous(memory_format=CL) and torch.equal(ga, gb)          # one pass serves both operands
    assert ref.check(f"{kind} {shape4} adjoint, k u sum |w g|", ga, y64, bound) <= 1.0
    _rule(f"{kind} {shape4} adjoint, the project's rule", ga, y64, y32)
    # the identity <R(a), g> = <a, R^T g> with the forward pass that ships
    gen = torch.Generator().manual_seed(1)
    a = torch.randn(shape, generator=gen)
    with torch.no_grad():
        Ra = A._resample_sum(kind, _nhwc(a), None)
    lhs, rhs = (Ra.double().cpu() * g.double()).sum().item(), (a.double() * ga.double().cpu()).sum().item()
    scale = (ref.resample(kind, a.double().abs()) * g.double().abs()).sum().item()
    print(f"{kind} {shape4} <R a, g> - <a, R^T g> = {lhs - rhs:.3e} ({abs(lhs - rhs) / (34 * ref.U * scale):.3f} of 34 u sum |R||a||g|)")
    assert abs(lhs - rhs) <= 34 * ref.U * scale          # (17 roundings a side at the most, see the ref's docstring)


def _one_hot_in_the_second_trip(kind, shape4):
    """The large shape, whose last rows of the last frame a thread of the adjoint reaches on its second trip of the grid-stride loop: g
    one-hot (all channels) in the last frame at outputs those rows hear from -- the bottom corners and two pixels further up, one of
    whose inputs straddle the two trips for "Down".  grad_in is the fp64 adjoint exactly -- zeros in all the rest, first trip included --
    and where it is not 0 it is the forward kernel's weight, read off a forward pass of one one-hot input per frame"""
    B, H, W, C = shape4
    total4, rest, rows = ref.second_trip(shape4)
    assert rest > 0 and rows == 4
    Ho, Wo = (2 * H, 2 * W) if kind == "Up" else (H // 2, W // 2)
    g = torch.zeros(B, C, Ho, Wo, device=DEV).contiguous(memory_format=CL)
    gin = torch.empty(B, C, H, W, device=DEV).contiguous(memory_format=CL)
    for Y, X in ((Ho - 1, 0), (Ho - 1, Wo - 1), (Ho - (6 if kind == "Up" else 2), Wo // 2), (Ho - 2, 1)):
        g[B - 1, :, Y, X] = 1.0
        gin.fill_(float("nan"))
        _lib.call("ps_upsample_add_bwd_nhwc_f32" if kind == "Up" else "ps_pool_add_bwd_nhwc_f32", g, B, H, W, C, gin)
        torch.cuda.synchronize()
        g[B - 1, :, Y, X] = 0.0
        one = torch.zeros(1, 1, Ho, Wo)
        one[0, 0, Y, X] = 1.0
        want = ref.adjoint(kind, one, (1, 1, H, W)).float()[0, 0]                       # (frames and channels are independent)
        heard = want.nonzero().tolist()
        assert 1 <= len(heard) <= 9 and min(y for y, _ in heard) >= H - rows - 1 and max(y for y, _ in heard) >= H - rows
        assert not gin[:B - 1].any() and torch.equal(gin[B - 1].cpu(), want.expand(C, H, W)), (Y, X)
        a = torch.zeros(len(heard), 4, H, W)
        for k, (y, x) in enumerate(heard):
            a[k, :, y, x] = 1.0
        with torch.no_grad():
            fwd = A._resample_sum(kind, _nhwc(a), None)[:, 0, Y, X].cpu()
        assert torch.equal(fwd, torch.stack([want[y, x] for y, x in heard])), (Y, X)


@pytest.mark.parametrize("kind,shape4", [("Up", ref.UP_SHAPES[1]), ("Up", ref.UP_SHAPES[2]), ("Down", ref.DOWN_SHAPES[1]), ("Down", ref.DOWN_SHAPES[2]),
                                         ("Up", ref.BIG_RESAMPLE), ("Down", ref.BIG_RESAMPLE)],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_one_hot_gradients_give_the_forwards_weights_exactly(kind, shape4):
    """g one-hot at the four corners of the output and at one interior pixel: grad_in[y][x] is the weight with which the forward kernel
    sends input (y, x) to that output -- read off the forward kernel itself, one one-hot input per frame -- and equals the fp64 adjoint"""
    if shape4 == ref.BIG_RESAMPLE:
        return _one_hot_in_the_second_trip(kind, shape4)
    _, H, W, _ = shape4
    eye = torch.eye(H * W).view(H * W, 1, H, W).expand(H * W, 4, H, W)
    with torch.no_grad():
        fwd = A._resample_sum(kind, _nhwc(eye), None)                      # fwd[y W + x, :, Y, X]: the weight of (y, x) in (Y, X)
    Ho, Wo = fwd.shape[2:]
    seen = set()
    for Y, X in ((0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1), (Ho // 2, Wo // 2)):
        g = torch.zeros(1, 4, Ho, Wo)
        g[0, :, Y, X] = 1.0
        got, _ = _adjoint(kind, g, (1, 4, H, W), b=False)
        want = fwd[:, :, Y, X].t().reshape(1, 4, H, W)
        assert torch.equal(got, want) and torch.equal(got.cpu(), ref.adjoint(kind, g, (1, 4, H, W)).float()), (Y, X)
        seen |= set(got.flatten().tolist())
    allowed = {0.0, 1.0, 0.75, 0.25, 0.5625, 0.1875, 0.0625} if kind == "Up" else {0.0, (torch.tensor(1.0) / 9).item()}
    assert seen <= allowed and (kind == "Down" or {0.5625, 0.1875, 0.0625, 1.0, 0.0} <= seen), seen


# ---- the 1 x 1 convolution ----------------------------------------------------------------------------------------------------------------
def _gw_case(shape):
    if shape not in _REFS:
        x, w, b, g = ref.gw_inputs(*shape)
        _REFS[shape] = (x, w, b, g, ref.conv1x1_grads(x, w, b, g), ref.conv1x1_grads(x, w, b, g, torch.float32))
    return _REFS[shape]


def _conv_backward(x, w, b, g, needs=(True, True, True)):
    dx, dw = _nhwc(x).requires_grad_(needs[0]), w.to(DEV).requires_grad_(needs[1])
    db = None if b is None else b.to(DEV).requires_grad_(needs[2])
    y = BT.conv1x1_train(dx, dw, db)
    assert y.requires_grad and y.is_contiguous(memory_format=CL)
    y.backward(_nhwc(g))
    torch.cuda.synchronize()
    return y.detach(), dx.grad, dw.grad, None if db is None else db.grad


@pytest.mark.parametrize("shape", ref.GW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_three_gradients_of_the_conv1x1_against_fp64(shape):
    npix, Ci, Co = shape
    parts = ref.part_ranges(*shape)
    assert len(parts) == _lib.call("ps_conv1x1_grad_weight_parts", *shape)
    if shape == ref.GW_SHAPES[0]:
        assert len(parts) == 1
    if shape == ref.GW_SHAPES[3]:
        assert len(parts) > 1 and parts[-1][1] - parts[-1][0] < parts[0][1] - parts[0][0]
    x, w, b, g, g64, g32 = _gw_case(shape)
    _, gx, gw, gb = _conv_backward(x, w, b, g)
    assert gx.shape == x.shape and gx.is_contiguous(memory_format=CL) and gw.shape == w.shape and gb.shape == b.shape
    for name, got, want, w32 in zip(("grad_input", "grad_weight", "grad_bias"), (gx, gw, gb), g64, g32):
        _rule(f"{shape} {name}", got, want, w32)
    L = ref.chain(*shape)
    assert ref.check(f"{shape} grad_weight, (L + parts) u sum |g||x| (L = {L}, parts = {len(parts)})", gw, g64[1],
                     ref.grad_weight_bound(x, g, *shape)) <= 1.0
    # a column of zeros in g: an exact-zero row of grad_weight and an exact 0 in grad_bias, the other rows as they were
    h = g.clone()
    h[:, 5] = 0
    _, _, hw, hb = _conv_backward(x, w, b, h)
    keep = [o for o in range(Co) if o != 5]
    assert not hw[5].any() and hb[5].item() == 0 and torch.equal(hw[keep], gw[keep]) and torch.equal(hb[keep], gb[keep])


def test_two_backward_runs_give_the_same_bits():
    shape = ref.GW_SHAPES[3]
    x, w, b, g = _gw_case(shape)[:4]
    first, second = _conv_backward(x, w, b, g), _conv_backward(x, w, b, g)
    assert all(torch.equal(p, q) for p, q in zip(first, second))
    for kind, shape4 in (("Up", ref.UP_SHAPES[2]), ("Down", ref.DOWN_SHAPES[2])):
        shp, gg = _adjoint_case(kind, shape4)[:2]
        assert torch.equal(_adjoint(kind, gg, shp)[0], _adjoint(kind, gg, shp)[0])


def test_the_forward_passes_are_the_no_grad_kernels():
    shape = ref.GW_SHAPES[2]
    x, w, b, g = _gw_case(shape)[:4]
    y = _conv_backward(x, w, b, g)[0]
    xd, Co, Ci = _nhwc(x), w.size(0), w.size(1)
    direct = torch.empty_like(y)
    _lib.call("ps_conv1x1_ex_nhwc_f32", xd, Ci, w.to(DEV).view(Co, Ci).contiguous(), b.to(DEV), None, 0, shape[0], Ci, Co, direct)
    assert torch.equal(y, direct)
    y2 = BT.conv1x1_train(xd, w.to(DEV).view(Co, Ci).requires_grad_())          # a 2-D weight, no bias
    conv = torch.nn.Conv2d(Ci, Co, 1, bias=False).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w)
        assert torch.equal(y2.detach(), A.conv1x1(conv, xd))
    gen = torch.Generator().manual_seed(2)
    for kind, (B, H, W, C) in (("Up", ref.UP_SHAPES[2]), ("Down", ref.DOWN_SHAPES[2])):
        a, c = (_nhwc(torch.randn(B, C, H, W, generator=gen)) for _ in range(2))
        with torch.no_grad():
            both, alone = A._resample_sum(kind, a, c), A._resample_sum(kind, a, None)
        assert torch.equal(BT.resample_sum_train(kind, a.clone().requires_grad_(), c).detach(), both)
        assert torch.equal(BT.resample_sum_train(kind, a.clone().requires_grad_(), None).detach(), alone)


def test_only_what_requires_grad_gets_a_gradient(monkeypatch):
    shape = ref.GW_SHAPES[1]
    x, w, b, g = _gw_case(shape)[:4]
    _, gx, gw, gb = _conv_backward(x, w, b, g)
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    for needs in ((False, True, False), (True, False, False), (False, False, True), (True, True, False)):
        del calls[:]
        _, hx, hw, hb = _conv_backward(x, w, b, g, needs)
        for full, got, need in ((gx, hx, needs[0]), (gw, hw, needs[1]), (gb, hb, needs[2])):
            assert (got is not None) == need and (not need or torch.equal(got, full)), needs
        # the forward's launch, then: the 1 x 1 kernel on g for the input alone, the GEMM for the weight or the bias alone
        assert calls.count("ps_conv1x1_nhwc_f32") == int(needs[0]) and calls.count("ps_conv1x1_grad_weight_f32") == int(needs[1] or needs[2]), needs
    _, hx, hw, hb = _conv_backward(x, w, None, g)
    assert hb is None and torch.equal(hx, gx) and torch.equal(hw, gw)
    # the join: a alone (b = None), and b without a
    for kind, shape4 in (("Up", ref.UP_SHAPES[1]), ("Down", ref.DOWN_SHAPES[1])):
        shp, gg = _adjoint_case(kind, shape4)[:2]
        ga, gb2 = _adjoint(kind, gg, shp)
        alone, none = _adjoint(kind, gg, shp, b=False)
        assert none is None and torch.equal(alone, ga)
        a = torch.zeros(shp, device=DEV).contiguous(memory_format=CL)
        c = a.clone().requires_grad_()
        del calls[:]
        BT.resample_sum_train(kind, a, c).backward(_nhwc(gg))
        assert a.grad is None and torch.equal(c.grad, gb2) and sum(n.endswith("_bwd_nhwc_f32") for n in calls) == 1


# ---- the decoder's blocks -----------------------------------------------------------------------------------------------------------------------
def _spy(monkeypatch):
    calls, real = [], _lib.call

    def call(name, *args, **kw):
        calls.append(name)
        return real(name, *args, **kw)
    monkeypatch.setattr(_lib, "call", call)
    return calls


def _block_gradients(blk, x, noise, proj):
    """-> (y, {name: gradient}) of sum(blk(x) * proj), 'input' among the names"""
    x = x.clone().requires_grad_()
    y = blk(x, noise)
    (y * proj).sum().backward()
    grads = {n: p.grad for n, p in blk.named_parameters()}
    grads["input"] = x.grad
    return y.detach(), grads


BLOCKS = {"Down": (64, 128, 8), "Up": (128, 64, 32)}          # kind -> (Ci, Co, side of the output) on a 16 x 16 input


def _block_case(kind, seed=0):
    Ci, Co, side = BLOCKS[kind]
    torch.manual_seed(seed)
    blk = A.ResNet_Block(Ci, Co, syn.network_opts(), kind).train()
    gen = torch.Generator().manual_seed(seed + 11)
    x = 0.3 + 1.5 * torch.randn(2, Ci, 16, 16, generator=gen)
    noise = [torch.randn(2, A.NOISE_SZ, generator=gen) for _ in range(2)]
    proj = torch.randn(2, Co, side, side, generator=gen)
    return blk, x, noise, proj


@pytest.mark.parametrize("kind", ["Down", "Up"])
def test_a_resampling_block_trains_with_no_torch_pass_over_an_activation(kind, monkeypatch):
    """Fails on the parent commit (there is no decoder_block_train).  Fully in train(), the convolutions on the fp16 matrix pipe, the norms,
    the 1 x 1 projection and the join through the three training libraries: against the fp64 twin on the host"""
    cpu, x, noise, proj = _block_case(kind)
    twin, dev = copy.deepcopy(cpu).double(), copy.deepcopy(cpu).to(DEV)
    y64, g64 = _block_gradients(twin, x.double(), [n.double() for n in noise], proj.double())
    y32, g32 = _block_gradients(cpu, x, noise, proj)
    calls = _spy(monkeypatch)
    f16x3.flag(DEV).zero_()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        with BT.decoder_block_train("hip"), f16x3.decoder_conv_train("f16x3"):
            y, got = _block_gradients(dev, _nhwc(x), [n.to(DEV) for n in noise], _nhwc(proj))
        torch.cuda.synchronize()
    adjoint, forward = ("ps_pool_add_bwd_nhwc_f32", "ps_pool_add_nhwc_f32") if kind == "Down" else ("ps_upsample_add_bwd_nhwc_f32", "ps_upsample_add_nhwc_f32")
    assert calls.count("ps_conv1x1_grad_weight_f32") == 1 and calls.count(adjoint) == 1 and calls.count(forward) == 1
    assert calls.count("ps_conv1x1_ex_nhwc_f32") == 1 and calls.count("ps_conv1x1_nhwc_f32") == 1           # forward; grad_input
    assert calls.count("ps_conv3x3_grad_weight_f16x3") == 2 and calls.count("ps_norm_train_backward_f32") == 2 and int(f16x3.flag(DEV).item()) == 0
    ops = {e.key for e in prof.key_averages()}
    banned = [k for k in ops if any(s in k for s in ("avg_pool2d", "upsample_bilinear2d", "convolution", "conv2d"))]
    assert not banned and "aten::avg_pool2d_backward" not in ops and "aten::upsample_bilinear2d_backward" not in ops, banned
    _rule(f"{kind} block output", y, y64, y32)
    assert set(got) == set(g64) and {"input", "ch_b.0.weight_orig", "ch_b.0.bias", "ch_a.5.weight_orig"} <= set(got)
    worst = max(_rule(f"{kind} {name}", got[name], g64[name], g32[name]) for name in sorted(got))
    print(f"{kind} block: largest gradient error / bound {worst:.3f}")


@pytest.mark.parametrize("kind", ["Down", "Up"])
def test_without_the_opt_in_nothing_changes(kind, monkeypatch):
    """The default: no export of the new library is called, and output and gradients are bit for bit those of a run in which the new
    module's Functions raise.  (The Down block's gradients: torch's upsample_bilinear2d_backward adds with atomics on the device, so two
    runs of the Up block's default route need not agree in their last bit; its output is compared.)"""
    monkeypatch.setattr(BT, "DECODER_BLOCK_TRAIN", "torch")
    cpu, x, noise, proj = _block_case(kind, seed=3)
    calls = _spy(monkeypatch)
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True       # (two runs of the same MIOpen convolutions: the same algorithm, no atomics)
    try:
        with f16x3.decoder_conv_train("f16x3"):
            y1, g1 = _block_gradients(copy.deepcopy(cpu).to(DEV), _nhwc(x), [n.to(DEV) for n in noise], _nhwc(proj))

            def refuse(*a, **k):
                raise AssertionError("the new route was taken without its opt-in")
            for name in ("conv1x1_train", "resample_sum_train"):
                monkeypatch.setattr(BT, name, refuse)
            monkeypatch.setattr(BT._Conv1x1Train, "apply", refuse)
            monkeypatch.setattr(BT._ResampleSum, "apply", refuse)
            y2, g2 = _block_gradients(copy.deepcopy(cpu).to(DEV), _nhwc(x), [n.to(DEV) for n in noise], _nhwc(proj))
    finally:
        torch.backends.cudnn.deterministic = was
    assert not [c for c in calls if c in _lib.BLOCK_TRAIN_PROTOS], calls
    assert torch.equal(y1, y2) and set(g1) == set(g2) and all(g1[n] is not None for n in g1)
    if kind == "Down":
        assert all(torch.equal(g1[n], g2[n]) for n in g1)


def test_ten_adam_steps_of_a_down_and_an_up_block():
    """Down, then Up, on a fixed 16 x 16 batch under all three HIP opt-ins (the norm's is the default): the loss falls"""
    torch.manual_seed(7)
    down = A.ResNet_Block(64, 128, syn.network_opts(), "Down").to(DEV).train()
    up = A.ResNet_Block(128, 64, syn.network_opts(), "Up").to(DEV).train()
    gen = torch.Generator().manual_seed(8)
    x = _nhwc(torch.randn(2, 64, 16, 16, generator=gen))
    target = _nhwc(torch.randn(2, 64, 16, 16, generator=gen)) * 0.5
    noise = [torch.randn(2, A.NOISE_SZ, generator=gen).to(DEV) for _ in range(4)]
    opt = torch.optim.Adam(list(down.parameters()) + list(up.parameters()), lr=2e-3)
    losses = []
    with BT.decoder_block_train("hip"), f16x3.decoder_conv_train("f16x3"), A.decoder_norm_train("hip"):
        for _ in range(10):
            opt.zero_grad()
            loss = (up(down(x, noise[:2]), noise[2:]) - target).square().mean()
            loss.backward()
            opt.step()
            losses.append(loss.item())
    print("losses", " ".join(f"{v:.5f}" for v in losses))
    assert all(v == v and abs(v) != float("inf") for v in losses) and losses[-1] < losses[0]
    f16x3.check_f16x3_overflow(DEV)
