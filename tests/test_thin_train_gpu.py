"""GPU: the decoder's thin first and last layers in training mode (csrc/thin_train.hip behind include/pixelsynth_thin_train.h, the
autograd Functions of networks/thin_train.py, the blocks' opt-in decoder_thin_train).

Operator level, at the smallest shapes at which each branch can go wrong (tests/_thin_train_ref.py lists them and derives the bounds):
the forward passes and the thin-in grad_input bit for bit against the no-grad kernels called directly, ps_thin_expand_f32 and
ps_thin_grad_weight_f32 under their bounds, every gradient under the project's rule, exact results where the arithmetic leaves no choice
(one-hot operands at corners and edges, a frame alone against the same frame in a batch, two runs).  Block level: the two thin blocks in
train() under all the opt-ins against their fp64 twins, the graph walked for the new Functions' nodes.  Decoder level: every parameter's
gradient against the fp64 twin with the thin-off route as the yardstick, ten Adam steps.  Every check prints its error / bound.
"""
import copy
import itertools

import pytest
import torch

import _thin_train_ref as ref
from pixelsynth_amd import _lib, synthetic as syn
from pixelsynth_amd.networks import architectures as A, block_train as BT, f16x3, thin_train as TT
from pixelsynth_amd.networks.routing import empty_nhwc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
_REFS = {}


def _nhwc(t):
    return t.to(DEV).contiguous(memory_format=CL)


def _rule(name, got, want64, got32=None, floor=None):
    bound, E32 = ref.grad_bound(got32, want64, floor)
    r = ref.check(f"{name} (yardstick {E32:.3e}, max |g64| {want64.abs().max().item():.3e})", got, want64, bound)
    assert r <= 1.0, name
    return r


def _case(kind, frame, wide, T, k):
    key = (kind, frame, wide, T, k)
    if key not in _REFS:
        x, w, b, g = ref.inputs(kind, frame, wide, T, k)
        _REFS[key] = (x, w, b, g, ref.conv_grads(x, w, b, g), ref.conv_grads(x, w, b, g, torch.float32))
    return _REFS[key]


def _backward(kind, x, w, b, g, needs=(True, True, True)):
    """-> (y, grad_input, grad_weight, grad_bias) of the Function of `kind` on device copies"""
    fn = TT.conv_thin_in_train if kind == "in" else TT.conv_thin_out_train
    dx, dw = _nhwc(x).requires_grad_(needs[0]), w.to(DEV).requires_grad_(needs[1])
    db = None if b is None else b.to(DEV).requires_grad_(needs[2])
    y = fn(dx, dw, db)
    assert y.requires_grad and y.is_contiguous(memory_format=CL) and y.shape == g.shape
    y.backward(_nhwc(g))
    torch.cuda.synchronize()
    return y.detach(), dx.grad, dw.grad, None if db is None else db.grad


def _kernel(kind, xd, wd):
    """The no-grad kernel of a thin layer, called directly: conv(xd, wd) without a bias.  kind "in": 4 -> Co, "out": Ci -> Co <= 4"""
    B, Ci, H, W = xd.shape
    Co, k = wd.size(0), wd.size(2)
    y = empty_nhwc(B, Co, H, W, xd)
    if k == 1:
        _lib.call("ps_conv1x1_nhwc_f32", xd, wd.reshape(Co, Ci).contiguous(), B * H * W, Ci, Co, y)
    elif kind == "in":
        _lib.call("ps_conv3x3_thin_in_nhwc_f32", xd, None, None, wd.permute(2, 3, 1, 0).contiguous(), B, H, W, Co, y)
    else:
        _lib.call("ps_conv3x3_thin_out_nhwc_f32", xd, None, None, wd.permute(2, 3, 1, 0).contiguous(), B, H, W, Ci, Co, y)
    torch.cuda.synchronize()
    return y


def _parts(frame, wide, T, k):
    """The number of parts the library reports, held to the restatement's; -> the restatement's ranges"""
    parts = ref.part_ranges(frame[0] * frame[1] * frame[2])
    assert _lib.call("ps_thin_train_parts", *frame, wide, T, k) == len(parts)
    assert _lib.call("ps_thin_train_workspace_bytes", *frame, wide, T, k) == ref.workspace_bytes(*frame, wide, T, k)
    if frame == ref.RAGGED:      # the shape chosen for it: at least two parts, and a shorter last one
        assert len(parts) >= 2 and parts[-1][1] - parts[-1][0] < parts[0][1] - parts[0][0]
    return parts


def _sums(tag, x, w, g, gw, gb, g64):
    """grad_weight and grad_bias under the chain rule of the restated layout"""
    npix = x.size(0) * x.size(2) * x.size(3)
    bw, bb = ref.sums_bound(x, w, g)
    L, parts = ref.chain(npix), len(ref.part_ranges(npix))
    assert ref.check(f"{tag} grad_weight, (L + parts) u sum |g||x| (L = {L}, parts = {parts})", gw, g64[1], bw) <= 1.0
    assert ref.check(f"{tag} grad_bias, (L + parts) u sum |g|", gb, g64[2], bb) <= 1.0


OUT_CASES = list(itertools.product(ref.FRAMES, ref.WIDE, ref.THIN_OUT, ref.KS)) + [(ref.RAGGED, 32, 3, 3), (ref.RAGGED, 128, 4, 1)]
IN_CASES = list(itertools.product(ref.FRAMES, ref.WIDE, ref.KS)) + [(ref.RAGGED, 32, 3), (ref.RAGGED, 64, 1)]
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


@pytest.mark.parametrize("frame,wide,T,k", OUT_CASES, ids=_ids)
def test_a_thin_out_layer(frame, wide, T, k):
    """wide -> T: the forward pass, ps_thin_expand_f32 (grad_input), ps_thin_grad_weight_f32 with the thin side as g"""
    _parts(frame, wide, T, k)
    x, w, b, g, g64, g32 = _case("out", frame, wide, T, k)
    tag = f"out {frame} {wide} -> {T}, k = {k}:"
    y, gx, gw, gb = _backward("out", x, w, b, g)
    assert torch.equal(y, _kernel("out", _nhwc(x), w.to(DEV)) + b.to(DEV).view(1, -1, 1, 1))          # the kernel's bits, one rounded add
    assert gx.shape == x.shape and gx.is_contiguous(memory_format=CL) and gw.shape == w.shape and gb.shape == b.shape
    assert ref.check(f"{tag} grad_input, n u sum |w g|", gx, g64[0], ref.expand_bound(x, w, g)) <= 1.0
    _sums(tag, x, w, g, gw, gb, g64)
    for name, got, want, w32 in zip(("grad_input", "grad_weight", "grad_bias"), (gx, gw, gb), g64, g32):
        _rule(f"{tag} {name}, the project's rule", got, want, w32)
    again = _backward("out", x, w, b, g)
    assert all(torch.equal(p, q) for p, q in zip((y, gx, gw, gb), again))                              # two runs, the same bits
    if frame[0] > 1:      # the last frame alone gives the bits it gives in the batch
        alone = _backward("out", x[-1:], w, b, g[-1:], (True, False, False))[1]
        assert torch.equal(alone[0], gx[-1])


@pytest.mark.parametrize("frame,wide,k", IN_CASES, ids=_ids)
def test_a_thin_in_layer(frame, wide, k):
    """4 -> wide: the forward pass, grad_input through the existing kernels on the flipped weight, ps_thin_grad_weight_f32 with the wide
    side as g"""
    _parts(frame, wide, 4, k)
    x, w, b, g, g64, g32 = _case("in", frame, wide, 4, k)
    tag = f"in {frame} 4 -> {wide}, k = {k}:"
    y, gx, gw, gb = _backward("in", x, w, b, g)
    wd = w.to(DEV)
    assert torch.equal(y, _kernel("in", _nhwc(x), wd) + b.to(DEV).view(1, -1, 1, 1))
    # grad_input: the thin-out / 1 x 1 kernel on g with the weight flipped and transposed, bit for bit
    assert gx.shape == x.shape and gx.is_contiguous(memory_format=CL) and gw.shape == w.shape and gb.shape == b.shape
    assert torch.equal(gx, _kernel("out", _nhwc(g), wd.flip(2, 3).transpose(0, 1).contiguous()))
    _sums(tag, x, w, g, gw, gb, g64)
    for name, got, want, w32 in zip(("grad_input", "grad_weight", "grad_bias"), (gx, gw, gb), g64, g32):
        _rule(f"{tag} {name}, the project's rule", got, want, w32)
    again = _backward("in", x, w, b, g)
    assert all(torch.equal(p, q) for p, q in zip((y, gx, gw, gb), again))


# ---- exact results ------------------------------------------------------------------------------------------------------------------------
H1, W1 = 8, 64
SPOTS = [(0, 0), (0, W1 - 1), (H1 - 1, 0), (H1 - 1, W1 - 1), (0, W1 // 2), (H1 - 1, 3), (H1 // 2, 0), (3, W1 - 1), (4, 4), (2, 31)]


@pytest.mark.parametrize("T,k", [(1, 3), (3, 3), (4, 3), (3, 1)], ids=_ids)
def test_a_one_hot_gradient_returns_the_weights_themselves(T, k):
    """The padding check of ps_thin_expand_f32: g one-hot (1.0 in the last thin channel) at each corner, on each edge and inside, one spot
    per frame -- grad_input is W[j][c][dy + r][dx + r] at (Y + dy, X + dx) where that is inside the frame and 0 elsewhere, exactly"""
    wide, r, j = 32, k // 2, T - 1
    x, w, b, _ = ref.inputs("out", (len(SPOTS), H1, W1), wide, T, k, seed=3)
    g = torch.zeros(len(SPOTS), T, H1, W1)
    want = torch.zeros(len(SPOTS), wide, H1, W1)
    for f, (Y, X) in enumerate(SPOTS):
        g[f, j, Y, X] = 1.0
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if 0 <= Y + dy < H1 and 0 <= X + dx < W1:
                    want[f, :, Y + dy, X + dx] = w[j, :, dy + r, dx + r]
    gx = _backward("out", x, w, b, g, (True, False, False))[1]
    assert torch.equal(gx.cpu(), want) and torch.equal(gx.cpu().double(), ref.conv_grads(x, w, b, g)[0])


# (the pixel Q of g's one, the pixel P of x's one, the tap (ky, kx) with P = Q + off(tap) or None where P is no neighbour of Q)
PAIRS = [((0, 0), (1, 1), (2, 2)), ((0, W1 - 1), (0, W1 - 2), (1, 0)), ((H1 - 1, 0), (H1 - 2, 0), (0, 1)), ((H1 - 1, W1 - 1), (H1 - 1, W1 - 1), (1, 1)),
         ((1, 0), (0, W1 - 1), None), ((3, W1 - 1), (4, 0), None), ((H1 - 1, W1 - 1), (0, 0), None)]


@pytest.mark.parametrize("kind", ["in", "out"])
def test_one_hot_operands_give_an_exact_product_in_the_right_tap(kind):
    """ps_thin_grad_weight_f32 with either operand as g: x one-hot (3.0) at P and g one-hot (0.5) at Q -- grad_weight is 1.5 in the tap
    that leads from Q to P and 0 everywhere else, also where P and Q are neighbours in memory only (the end of one row and the start of
    the next, the last pixel of one frame and the first of the next); grad_bias is 0.5 in g's channel"""
    wide, T = 64, (4 if kind == "in" else 3)
    Ci, Co = (4, wide) if kind == "in" else (wide, T)
    ci, co = Ci - 1, Co - 2
    w, b = torch.zeros(Co, Ci, 3, 3), torch.zeros(Co)
    for Q, P, tap in PAIRS:
        last = Q == (H1 - 1, W1 - 1) and P == (0, 0)               # g's one in frame 0, x's in frame 1
        x, g = torch.zeros(2, Ci, H1, W1), torch.zeros(2, Co, H1, W1)
        x[1 if last else 0, ci, P[0], P[1]] = 3.0
        g[0, co, Q[0], Q[1]] = 0.5
        _, _, gw, gb = _backward(kind, x, w, b, g, (False, True, True))
        want = torch.zeros_like(w)
        if tap is not None:
            want[co, ci, tap[0], tap[1]] = 1.5
        want_b = torch.zeros(Co)
        want_b[co] = 0.5
        assert torch.equal(gw.cpu(), want) and torch.equal(gb.cpu(), want_b), (kind, Q, P)
        assert torch.equal(want.double(), ref.conv_grads(x, w, b, g)[1])


def test_only_what_requires_grad_gets_a_gradient(monkeypatch):
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    for kind in ("in", "out"):
        x, w, b, g = _case(kind, ref.FRAMES[1], 64, 4 if kind == "in" else 3, 3)[:4]
        _, gx, gw, gb = _backward(kind, x, w, b, g)
        for needs in ((False, True, False), (True, False, False), (False, False, True), (True, True, False)):
            del calls[:]
            _, hx, hw, hb = _backward(kind, x, w, b, g, needs)
            for full, got, need in ((gx, hx, needs[0]), (gw, hw, needs[1]), (gb, hb, needs[2])):
                assert (got is not None) == need and (not need or torch.equal(got, full)), (kind, needs)
            assert calls.count("ps_thin_grad_weight_f32") == int(needs[1] or needs[2])
            assert calls.count("ps_thin_expand_f32") == int(needs[0] and kind == "out")
            assert calls.count("ps_conv3x3_thin_out_nhwc_f32") == int(kind == "out") + int(needs[0] and kind == "in")
        _, hx, hw, hb = _backward(kind, x, w, None, g)
        assert hb is None and torch.equal(hx, gx) and torch.equal(hw, gw)


# ---- the decoder's thin blocks ------------------------------------------------------------------------------------------------------------
def _block_gradients(blk, x, noise, proj):
    """-> (y, {name: gradient}, the names of the autograd nodes behind y) of sum(blk(x) * proj), 'input' among the names"""
    x = x.clone().requires_grad_()
    y = blk(x, noise)
    seen, todo, names = set(), [y.grad_fn], []
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        todo.extend(f for f, _ in fn.next_functions)
    (y * proj).sum().backward()
    grads = {n: p.grad for n, p in blk.named_parameters()}
    grads["input"] = x.grad
    return y.detach(), grads, names


def _thin_nodes(names):
    return sorted(n for n in names if "ConvThin" in n)


@pytest.mark.parametrize("ends", [(4, 64), (128, 3)], ids=_ids)
def test_a_thin_block_trains_through_the_new_functions(ends, monkeypatch):
    """Fails on the parent commit (there is no decoder_thin_train).  ResNet_Block(4, 64) and ResNet_Block(128, 3) in train() on 2 x 8 x 64
    with every opt-in on: the graph behind the output holds the new Functions' nodes -- the 3 x 3 of branch a and the 1 x 1 projection --,
    none with the thin opt-in off, and every gradient is within the rule of the fp64 twin's, the same block in fp32 on the host as the
    yardstick"""
    monkeypatch.setattr(TT, "DECODER_THIN_TRAIN", "torch")
    torch.manual_seed(1)
    cpu = A.ResNet_Block(ends[0], ends[1], syn.network_opts()).train()
    gen = torch.Generator().manual_seed(12)
    x = 0.3 + 1.5 * torch.randn(2, ends[0], 8, 64, generator=gen)
    noise = [torch.randn(2, A.NOISE_SZ, generator=gen) for _ in range(2)]
    proj = torch.randn(2, ends[1], 8, 64, generator=gen)
    y64, g64, _ = _block_gradients(copy.deepcopy(cpu).double(), x.double(), [n.double() for n in noise], proj.double())
    y32, g32, host_names = _block_gradients(copy.deepcopy(cpu), x, noise, proj)
    dev_args = (_nhwc(x), [n.to(DEV) for n in noise], _nhwc(proj))
    f16x3.flag(DEV).zero_()
    with BT.decoder_block_train("hip"), f16x3.decoder_conv_train("f16x3"), A.decoder_norm_train("hip"):
        with TT.decoder_thin_train("hip"):
            y, got, names = _block_gradients(copy.deepcopy(cpu).to(DEV), *dev_args)
        _, _, names_off = _block_gradients(copy.deepcopy(cpu).to(DEV), *dev_args)              # the default: "torch"
        with TT.decoder_thin_train("torch"):
            _, _, names_forced = _block_gradients(copy.deepcopy(cpu).to(DEV), *dev_args)
    torch.cuda.synchronize()
    node = "_ConvThinInTrainBackward" if ends[0] == 4 else "_ConvThinOutTrainBackward"
    assert _thin_nodes(names) == [node, node], _thin_nodes(names)
    assert not _thin_nodes(names_off) and not _thin_nodes(names_forced) and not _thin_nodes(host_names)
    assert int(f16x3.flag(DEV).item()) == 0
    _rule(f"{ends} block output", y, y64, y32)
    assert set(got) == set(g64) and {"input", "ch_a.2.weight_orig", "ch_a.2.bias", "ch_b.0.weight_orig", "ch_b.0.bias"} <= set(got)
    worst = max(_rule(f"{ends} {name}", got[name], g64[name], g32[name]) for name in sorted(got))
    print(f"{ends} block: largest gradient error / bound {worst:.3f}")


# ---- the whole decoder --------------------------------------------------------------------------------------------------------------------
def _decoder_case():
    """A ResNetDecoder (256W8UpDown64, ngf = 64) in train() on 1 x 64 x 64 with fixed noise, its fp64 twin's gradients (computed once)"""
    if "decoder" not in _REFS:
        torch.manual_seed(2)
        opt = syn.network_opts(refine_model_type="resnet_256W8UpDown64", ngf=64, predict_residual=False)
        cpu = A.ResNetDecoder(opt, channels_in=64).train()
        gen = torch.Generator().manual_seed(13)
        x = torch.randn(1, 64, 64, 64, generator=gen)
        noise = [torch.randn(1, A.NOISE_SZ, generator=gen) for _ in range(cpu.n_noise())]
        proj = torch.randn(1, 3, 64, 64, generator=gen)
        _REFS["decoder"] = (cpu, x, noise, proj, _decoder_gradients(copy.deepcopy(cpu).double(), x.double(), [n.double() for n in noise], proj.double()))
    return _REFS["decoder"]


def _decoder_gradients(dec, x, noise, proj):
    x = x.clone().requires_grad_()
    (dec(x, noise=noise) * proj).sum().backward()
    grads = {n: p.grad for n, p in dec.named_parameters()}
    grads["input"] = x.grad
    return grads


def _all_on():
    return BT.decoder_block_train("hip"), f16x3.decoder_conv_train("f16x3"), A.decoder_norm_train("hip")


def test_a_whole_decoder_against_its_fp64_twin_with_the_parent_route_as_the_yardstick(monkeypatch):
    """All four opt-ins on against only the thin one off: for every parameter (and the input) the new route's error against the fp64 twin
    is at most 4 max(E_parent, 1e-6 max |g64|), E_parent the error of the thin-off run"""
    cpu, x, noise, proj, g64 = _decoder_case()
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    runs = {}
    for thin in ("hip", "torch"):
        del calls[:]
        a, b, c = _all_on()
        with a, b, c, TT.decoder_thin_train(thin):
            runs[thin] = _decoder_gradients(copy.deepcopy(cpu).to(DEV), x.to(DEV), [n.to(DEV) for n in noise], proj.to(DEV))
        torch.cuda.synchronize()
        # block 7's 128 -> 3 layers, 3 x 3 and 1 x 1: one weight gradient and one expansion each
        assert calls.count("ps_thin_grad_weight_f32") == calls.count("ps_thin_expand_f32") == (2 if thin == "hip" else 0)
    f16x3.check_f16x3_overflow(DEV)
    assert set(runs["hip"]) == set(g64) and all(v is not None for v in runs["hip"].values())
    worst = 0.0
    for name in sorted(g64):
        E_parent = (runs["torch"][name].double().cpu() - g64[name]).abs().max().item()
        worst = max(worst, _rule(f"decoder {name}", runs["hip"][name], g64[name], floor=E_parent))
    print(f"decoder: largest gradient error / bound {worst:.3f}")


def test_ten_adam_steps_of_the_decoder():
    """That decoder on a fixed input under all four opt-ins: the loss falls"""
    cpu, x, noise, proj, _ = _decoder_case()
    dec = copy.deepcopy(cpu).to(DEV)
    xd, nd = x.to(DEV), [n.to(DEV) for n in noise]
    target = torch.tanh(_nhwc(proj)) * 0.5
    opt = torch.optim.Adam(dec.parameters(), lr=2e-4)
    losses = []
    a, b, c = _all_on()
    with a, b, c, TT.decoder_thin_train("hip"):
        for _ in range(10):
            opt.zero_grad()
            loss = (dec(xd, noise=nd) - target).square().mean()
            loss.backward()
            opt.step()
            losses.append(loss.item())
    print("losses", " ".join(f"{v:.5f}" for v in losses))
    assert all(v == v and abs(v) != float("inf") for v in losses) and losses[-1] < losses[0]
    f16x3.check_f16x3_overflow(DEV)
