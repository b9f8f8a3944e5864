"""GPU: the VQ-VAE's training convolutions (csrc/vq_conv_train.hip, vqvae2/conv_train.py) and the route VQVAETop.forward takes under
vqvae_train("hip"), against the references and bounds of tests/_vq_conv_train_ref.py (rules 1 and 2 of tests/_conv_bwd_ref.py, the chain
bound of tests/_thin_train_ref.py, the gather bound of tests/_block_train_ref.py).  Every forward is held bit for bit to what the
inference fast path computes on the same weights, every output to the same bits on a second run, and frame 1 of 3 to the bits of the
same frame alone.  (The backward pass scales a layer's output gradient by a power of two chosen from the BATCH's largest magnitude, exact
down to fp16's normal range; the frame tests put the batch's largest gradient into frame 1 so that both runs choose the same power.)"""
import copy

import pytest
import torch
import torch.nn.functional as F

import _conv_bwd_ref as cref
import _vq_conv_train_ref as ref
from pixelsynth_amd import _lib
from pixelsynth_amd.networks import f16x3
from pixelsynth_amd.vqvae2 import conv_train as CT, train as vq_train, vqvae as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = torch.double


def nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same_values(a, b):
    """same_bits, a NaN matching any NaN (which NaN torch's relu hands back is not the point)"""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and same_bits(torch.nan_to_num(a, nan=0.0, posinf=None, neginf=None), torch.nan_to_num(b, nan=0.0, posinf=None, neginf=None))


def run(fn, x, params, g, *args, **kw):
    """fn(x, *params, *args) forward and backward on the device -> (y, [grad x, grad params ...])"""
    xg = nhwc(x).requires_grad_()
    leaves = [p.to(DEV).requires_grad_() for p in params]
    y = fn(xg, *leaves, *args, **kw)
    return y.detach(), list(torch.autograd.grad(y, [xg] + leaves, nhwc(g)))


def twice_and_frame(fn, x, params, g, first, *args, **kw):
    """A second run gives the same bits; with three frames, frame 1 alone gives its forward result and input gradient"""
    y, grads = first
    y2, grads2 = run(fn, x, params, g, *args, **kw)
    assert same_bits(y, y2) and all(same_bits(a, b) for a, b in zip(grads, grads2))
    if x.size(0) == 3:
        y1, grads1 = run(fn, x[1:2], params, g[1:2], *args, **kw)
        assert same_bits(y[1:2], y1) and same_bits(grads[0][1:2], grads1[0])


# ---- the stride-2 forms --------------------------------------------------------------------------------------------------------------------
S2_SHAPES = [(1, 64, 32, 32, 128), (2, 128, 32, 64, 128), (3, 64, 64, 32, 64)]          # (B, Ci, H, W, Co), the input's sides
T_SHAPES = [(1, 128, 16, 16, 64), (2, 64, 16, 32, 64), (3, 64, 32, 16, 64)]


def stride2_inputs(shape, transposed, seed=0):
    B, Ci, H, W, Co = shape
    gen = torch.Generator().manual_seed(4321 + seed + 7 * Ci + Co + H + 2 * transposed)
    x = 1.5 * torch.randn(B, Ci, H, W, generator=gen)
    w = torch.randn(*((Ci, Co) if transposed else (Co, Ci)), 4, 4, generator=gen) / ((2 if transposed else 4) * Ci ** 0.5)
    b = torch.randn(Co, generator=gen)
    g = torch.randn(B, Co, *((2 * H, 2 * W) if transposed else (H // 2, W // 2)), generator=gen)
    if B == 3:
        g[1, 0, 0, 0] = 7.5          # the batch's largest gradient lies in frame 1 (module docstring)
    return x, w, b, g


def forward_of_the_pack(x, w, b, relu_in, form):
    """f16x3.conv3x3 on the pack the fast path builds for this layer"""
    xg, wg, bg = nhwc(x), w.to(DEV), b.to(DEV)
    if form == "d2s":
        p = f16x3.pack3x3(V.convt_weight(wg), bg.repeat(4), d2s=True)
    else:
        p = f16x3.pack3x3(V.s2d_weight(wg), bg, s2d=form == "s2d")
    return f16x3.conv3x3(xg, p, *(f16x3.plain_relu(x.size(0), p["Ci"], DEV) if relu_in else ()))


def check_all(name, grads, r):
    for what, y, want in zip(("grad_input", "grad_weight", "grad_bias"), grads, (r.x, r.weight, r.bias)):
        cref.check(f"{name} {what}", y, want)


@pytest.mark.parametrize("relu_in", [True, False])
@pytest.mark.parametrize("shape", S2_SHAPES)
def test_conv4x4s2_train(shape, relu_in):
    x, w, b, g = stride2_inputs(shape, False)
    first = run(CT.conv4x4s2_train, x, (w, b), g, relu_in)
    y, grads = first
    assert same_bits(y, forward_of_the_pack(x, w, b, relu_in, "s2d"))
    check_all(f"conv4x4s2 {shape} relu {relu_in}", grads, ref.stride2_reference(x, w, g, relu_in, False))
    if relu_in:
        assert not grads[0][nhwc(x) <= 0].any()
    twice_and_frame(CT.conv4x4s2_train, x, (w, b), g, first, relu_in)


def test_conv4x4s2_train_on_a_blocked_input():
    x, w, b, g = stride2_inputs(S2_SHAPES[0], False, seed=1)
    xb = V._s2d(x)                                                    # what the stem leaves: (B, 4 Ci, H / 2, W / 2)
    y, grads = run(CT.conv4x4s2_train, xb, (w, b), g, True, x_is_s2d=True)
    assert same_bits(y, forward_of_the_pack(xb, w, b, True, "blocked"))
    r = ref.stride2_reference(x, w, g, True, False)
    blocked = cref.Gradient(*(V._s2d(t).contiguous() for t in (r.x.T, r.x.S, r.x.y32, r.x.g64)), r.x.E32)
    check_all("conv4x4s2 blocked", grads, cref.Reference(blocked, r.weight, r.bias, r.s))
    y2, grads2 = run(CT.conv4x4s2_train, xb, (w, b), g, True, x_is_s2d=True)
    assert same_bits(y, y2) and all(same_bits(a, c) for a, c in zip(grads, grads2))


@pytest.mark.parametrize("relu_in", [True, False])
@pytest.mark.parametrize("shape", T_SHAPES)
def test_convt4x4s2_train(shape, relu_in):
    x, w, b, g = stride2_inputs(shape, True)
    first = run(CT.convt4x4s2_train, x, (w, b), g, relu_in)
    y, grads = first
    assert same_bits(y, forward_of_the_pack(x, w, b, relu_in, "d2s"))
    check_all(f"convt4x4s2 {shape} relu {relu_in}", grads, ref.stride2_reference(x, w, g, relu_in, True))
    if relu_in:
        assert not grads[0][nhwc(x) <= 0].any()
    twice_and_frame(CT.convt4x4s2_train, x, (w, b), g, first, relu_in)


def test_small_gradients_run_through_both_stride2_forms():
    x, w, b, _ = stride2_inputs(S2_SHAPES[0], False, seed=2)
    g = cref.small_gradients(1, 16, 16, 64, 128)[3]
    _, grads = run(CT.conv4x4s2_train, x, (w, b), g, True)
    check_all("conv4x4s2 small g", grads, ref.stride2_reference(x, w, g, True, False))
    x, w, b, _ = stride2_inputs(T_SHAPES[0], True, seed=2)
    g = cref.small_gradients(1, 32, 32, 64, 64)[3]
    _, grads = run(CT.convt4x4s2_train, x, (w, b), g, True)
    check_all("convt4x4s2 small g", grads, ref.stride2_reference(x, w, g, True, True))


# ---- the stride-1 layers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu_in", [True, False])
def test_conv3x3_relu_train(relu_in):
    B, Ci, H, W, Co = 2, 64, 16, 16, 128
    gen = torch.Generator().manual_seed(11)
    x, w = 1.5 * torch.randn(B, Ci, H, W, generator=gen), torch.randn(Co, Ci, 3, 3, generator=gen) / (3 * Ci ** 0.5)
    b, g = torch.randn(Co, generator=gen), torch.randn(B, Co, H, W, generator=gen)
    first = run(CT.conv3x3_relu_train, x, (w, b), g, relu_in)
    y, grads = first
    p = f16x3.pack3x3(w.to(DEV), b.to(DEV))
    assert same_bits(y, f16x3.conv3x3(nhwc(x), p, *(f16x3.plain_relu(B, Ci, DEV) if relu_in else ())))
    check_all(f"conv3x3 relu {relu_in}", grads, ref.plain_reference(x, w, g, relu_in))
    if relu_in:
        assert not grads[0][nhwc(x) <= 0].any()
    twice_and_frame(CT.conv3x3_relu_train, x, (w, b), g, first, relu_in)


def autograd_on_the_host(f, leaves, g, dtype):
    leaves = [t.detach().to(dtype).clone().requires_grad_() for t in leaves]
    return torch.autograd.grad(f(*leaves), leaves, g.to(dtype))


def test_conv1x1_relu_train():
    B, Ci, H, W, Co = 2, 128, 16, 16, 64
    gen = torch.Generator().manual_seed(12)
    x, w = 1.5 * torch.randn(B, Ci, H, W, generator=gen), torch.randn(Co, Ci, 1, 1, generator=gen) / Ci ** 0.5
    b, g = torch.randn(Co, generator=gen), torch.randn(B, Co, H, W, generator=gen)
    first = run(CT.conv1x1_relu_train, x, (w, b), g)
    y, grads = first
    y0 = torch.empty_like(y)
    _lib.call("ps_conv1x1_ex_nhwc_f32", nhwc(x), Ci, w.reshape(Co, Ci).to(DEV), b.to(DEV), None, 1, B * H * W, Ci, Co, y0)
    assert same_bits(y, y0)

    def f(x, w, b):
        return F.conv2d(F.relu(x), w, b)
    g64, g32 = autograd_on_the_host(f, (x, w, b), g, D), autograd_on_the_host(f, (x, w, b), g, torch.float32)
    for what, got, a, c in zip(("grad_input", "grad_weight", "grad_bias"), grads, g64, g32):
        ref.rule2(f"conv1x1 relu {what}", got, a, c)
    assert not grads[0][nhwc(x) <= 0].any()
    twice_and_frame(CT.conv1x1_relu_train, x, (w, b), g, first)


class _Block:          # what ref._res reads of a ResBlock
    def __init__(self, w3, b3, w1, b1):
        self.conv = [None, type("L", (), dict(weight=w3, bias=b3)), None, type("L", (), dict(weight=w1, bias=b1))]


@pytest.mark.parametrize("B", [1, 3])
def test_res_block_train(B):
    C, H, W, mid = 128, 16, 16, 32
    gen = torch.Generator().manual_seed(13 + B)
    x = 1.5 * torch.randn(B, C, H, W, generator=gen)
    w3, b3 = torch.randn(mid, C, 3, 3, generator=gen) / (3 * C ** 0.5), torch.randn(mid, generator=gen)
    w1, b1 = torch.randn(C, mid, 1, 1, generator=gen) / mid ** 0.5, torch.randn(C, generator=gen)
    g = torch.randn(B, C, H, W, generator=gen)
    if B == 3:
        g[1, 0, 0, 0] = 7.5
    params = (w3, b3, w1, b1)
    first = run(CT.res_block_train, x, params, g)
    y, grads = first
    # the forward: _FastPath.res on the fast path's own packs
    fast = V._FastPath.__new__(V._FastPath)
    fast.device, fast.ones, fast.zeros = torch.device(DEV), {}, {}
    c3 = f16x3.pack3x3(w3.to(DEV), b3.to(DEV))
    assert same_bits(y, fast.res(nhwc(x), dict(c3=c3, w1=w1.reshape(C, mid).to(DEV).contiguous(), b1=b1.to(DEV))))
    # the gradients against the fp64 block on the run's own ReLU decisions
    h = fast.conv3(nhwc(x), c3, True)[:, :mid]
    masks = [(x > 0), (h > 0).cpu()]
    out = []
    for dtype in (D, torch.float32):
        mk = ref.Masks(masks)
        leaves = [t.to(dtype).clone().requires_grad_() for t in (x,) + params]
        blk = _Block(*leaves[1:])
        P = {id(t): t for t in leaves[1:]}
        out.append(torch.autograd.grad(ref._res(leaves[0], blk, P, mk, dtype == D), leaves, g.to(dtype)))
        if dtype == D:
            print(f"res block: {mk.flipped} of {mk.total} ReLU decisions differ from the fp64 block's own signs, {mk.near} near zero")
    for what, got, a, c in zip(("grad_input", "grad_w3", "grad_b3", "grad_w1", "grad_b1"), grads, *out):
        ref.rule2(f"res block B {B} {what}", got, a, c)
    assert not grads[0][nhwc(x) <= 0].any()
    twice_and_frame(CT.res_block_train, x, params, g, first)


# ---- the pack, gate and fold kernels, bit for bit against the torch expressions on the device ------------------------------------------------
def test_the_pack_gate_and_fold_kernels():
    gen = torch.Generator().manual_seed(14)
    B, C, H, W = 3, 12, 6, 10                      # 540 float4s: two workgroups and a partial third
    x = torch.randn(B, C, H, W, generator=gen)
    x[0, 1, 2, 3], x[2, 11, 5, 9], x[1, 0, 0, 0] = float("nan"), float("inf"), 0.0
    xg = nhwc(x)
    for relu in (False, True):
        a = torch.relu(xg) if relu else xg
        assert same_values(CT.relu_pack(xg, relu, False).permute(0, 2, 3, 1), a.permute(0, 2, 3, 1))
        assert same_values(CT.relu_pack(xg, relu, True).permute(0, 2, 3, 1), V._s2d(a).permute(0, 2, 3, 1))
    g, skip = nhwc(torch.randn(B, C, H, W, generator=gen)), nhwc(torch.randn(B, C, H, W, generator=gen))
    scale2 = torch.tensor([2.0 ** 13, 2.0 ** -13], device=DEV)
    zero = torch.zeros((), device=DEV)
    for m in (None, xg):
        for s in (None, skip):
            for sc in (None, scale2):
                want = g if sc is None else g * sc[1]
                want = want if s is None else want + s
                want = want if m is None else torch.where(m > 0, want, zero)
                got = CT.gate(g.clone(memory_format=torch.preserve_format), m, s, sc)
                assert same_bits(got.permute(0, 2, 3, 1), want.permute(0, 2, 3, 1)), (m is None, s is None, sc is None)
    for Co, Ci in ((5, 3), (20, 7)):               # 240 elements: one partial workgroup; 2240: eight and a partial ninth
        g3 = torch.randn(Co, 3, 3, 4 * Ci, generator=gen)
        assert torch.equal(CT.fold(g3.to(DEV), Co, Ci, False).cpu(), ref.fold_kernel_layout(g3, False))
        g3 = torch.randn(4 * Co, 3, 3, Ci, generator=gen)
        assert torch.equal(CT.fold(g3.to(DEV), Co, Ci, True).cpu(), ref.fold_kernel_layout(g3, True))


# ---- the ends ----------------------------------------------------------------------------------------------------------------------------
def bias_bound(t, P):
    return 1.01 * (ref.chain(P) + len(ref.part_ranges(P))) * ref.U * t


@pytest.mark.parametrize("shape", [(1, 3, 4, 16), (2, 3, 32, 48), (5, 3, 8, 64)])
def test_stem_train(shape):
    B, _, H, W = shape
    gen = torch.Generator().manual_seed(15 + H)
    img, w, b = 1.5 * torch.randn(*shape, generator=gen), torch.randn(64, 3, 4, 4, generator=gen) / 48 ** 0.5, torch.randn(64, generator=gen)
    g = torch.randn(B, 64, H // 2, W // 2, generator=gen)
    gb_ = nhwc(V._s2d(g))                                             # the gradient in the stem's own output form

    def once(img):
        leaves = [t.to(DEV).requires_grad_() for t in (w, b)]
        s = CT.stem_train(img.to(DEV), *leaves)
        return s.detach(), torch.autograd.grad(s, leaves, gb_[:img.size(0)])
    s, (gw, gbias) = once(img)
    s0 = torch.empty(B, H // 4, W // 4, 256, device=DEV)
    _lib.call("ps_vq_stem_s2d_f32", img.to(DEV), w.to(DEV), b.to(DEV), B, H, W, s0)
    assert same_bits(s.permute(0, 2, 3, 1), s0)
    P = B * (H // 2) * (W // 2)
    ref.within(f"stem {shape} grad_weight (chain bound)", gw, ref.ends_dw(img.double(), g.double()), ref.ends_bound(img, g))
    ref.rule2(f"stem {shape} grad_weight", gw, ref.ends_dw(img.double(), g.double()), ref.ends_dw(img, g))
    ref.within(f"stem {shape} grad_bias (chain bound)", gbias, g.double().sum((0, 2, 3)), bias_bound(g.double().abs().sum((0, 2, 3)), P))
    ref.rule2(f"stem {shape} grad_bias", gbias, g.double().sum((0, 2, 3)), g.sum((0, 2, 3)))
    s2, (gw2, gbias2) = once(img)
    assert same_bits(s, s2) and same_bits(gw, gw2) and same_bits(gbias, gbias2)
    if B >= 3:
        assert same_bits(once(img[1:2])[0], s[1:2])


@pytest.mark.parametrize("shape", [(1, 1, 16), (2, 8, 32), (3, 16, 16)])
def test_head_train(shape):
    B, Hh, Wh = shape
    gen = torch.Generator().manual_seed(16 + Hh)
    h, wt, b = 1.5 * torch.randn(B, 64, Hh, Wh, generator=gen), torch.randn(64, 3, 4, 4, generator=gen) / 16, torch.randn(3, generator=gen)
    g = torch.randn(B, 3, 2 * Hh, 2 * Wh, generator=gen)

    def once(h, g):
        leaves = [nhwc(h).requires_grad_()] + [t.to(DEV).requires_grad_() for t in (wt, b)]
        img = CT.head_train(*leaves)
        return img.detach(), torch.autograd.grad(img, leaves, g.to(DEV))
    img, (gh, gw, gbias) = once(h, g)
    img0 = torch.empty_like(img)
    _lib.call("ps_vq_head_f32", nhwc(h), wt.to(DEV), b.to(DEV), B, Hh, Wh, img0)
    assert same_bits(img, img0)
    mask = (h > 0)
    rh = torch.relu(h)
    ref.within(f"head {shape} grad_input (gather bound)", gh, ref.head_gin(g.double(), wt.double()) * mask, ref.head_gin_bound(g, wt))
    ref.rule2(f"head {shape} grad_input", gh, ref.head_gin(g.double(), wt.double()) * mask, ref.head_gin(g, wt) * mask)
    assert not gh[nhwc(h) <= 0].any()
    P = B * Hh * Wh
    ref.within(f"head {shape} grad_weight (chain bound)", gw, ref.ends_dw(g.double(), rh.double()), ref.ends_bound(g, rh))
    ref.rule2(f"head {shape} grad_weight", gw, ref.ends_dw(g.double(), rh.double()), ref.ends_dw(g, rh))
    ref.within(f"head {shape} grad_bias (chain bound)", gbias, g.double().sum((0, 2, 3)), bias_bound(g.double().abs().sum((0, 2, 3)), P))
    ref.rule2(f"head {shape} grad_bias", gbias, g.double().sum((0, 2, 3)), g.sum((0, 2, 3)))
    img2, grads2 = once(h, g)
    assert same_bits(img, img2) and all(same_bits(a, c) for a, c in zip((gh, gw, gbias), grads2))
    if B == 3:
        img1, (gh1, _, _) = once(h[1:2], g[1:2])
        assert same_bits(img[1:2], img1) and same_bits(gh[1:2], gh1)


def test_one_hot_operands_at_the_corners_and_on_an_edge():
    gen = torch.Generator().manual_seed(17)
    Hh, Wh = 4, 16
    H, W = 2 * Hh, 2 * Wh
    img, wt = torch.randn(1, 3, H, W, generator=gen), torch.randn(64, 3, 4, 4, generator=gen)
    pad = F.pad(img, (1, 1, 1, 1))
    for y, x in ((0, 0), (0, Wh - 1), (Hh - 1, 0), (Hh - 1, Wh - 1), (2, Wh - 1)):
        o = (5 * y + x) % 64
        wide = torch.zeros(1, 64, Hh, Wh)
        wide[0, o, y, x] = 1.0
        want = torch.zeros(64, 3, 4, 4)
        want[o] = pad[0, :, 2 * y:2 * y + 4, 2 * x:2 * x + 4]         # img[c, 2 y - 1 + ky, 2 x - 1 + kx], zeros outside the frame
        gw, gb = CT._ends_grad_weight(img.to(DEV), nhwc(wide), 1, H, W, False, True)
        assert torch.equal(gw.cpu(), want) and same_bits(gb.cpu(), img.double().sum((0, 2, 3)).float())
        gw, gb = CT._ends_grad_weight(img.to(DEV), nhwc(V._s2d(wide)), 1, H, W, True, True)
        assert torch.equal(gw.cpu(), want) and torch.equal(gb.cpu(), wide.sum((0, 2, 3)))
    ones = nhwc(torch.ones(1, 64, Hh, Wh))
    for Y, X in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (3, 0)):
        c = (Y + X) % 3
        g = torch.zeros(1, 3, H, W)
        g[0, c, Y, X] = 1.0
        gh = torch.empty_like(ones)
        _lib.call("ps_vq_head_grad_input_f32", g.to(DEV), wt.to(DEV), ones, 1, Hh, Wh, gh)
        want = torch.zeros(1, 64, Hh, Wh)
        for y in range(Hh):
            for x in range(Wh):
                ky, kx = Y - 2 * y + 1, X - 2 * x + 1
                if 0 <= ky <= 3 and 0 <= kx <= 3:
                    want[0, :, y, x] = wt[:, c, ky, kx]
        assert torch.equal(gh.cpu(), want)


# ---- the network ---------------------------------------------------------------------------------------------------------------------------
NAMES = ("conv3x3_relu_train", "conv4x4s2_train", "convt4x4s2_train", "res_block_train", "conv1x1_relu_train", "stem_train", "head_train",
         "conv1x1_train")


def network(seed=0):
    torch.manual_seed(seed)
    m = V.VQVAETop().to(DEV).train()
    x = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
    return m, x


def spy(monkeypatch):
    counts = dict.fromkeys(NAMES, 0)

    def wrap(name, fn):
        def f(*a, **k):
            counts[name] += 1
            return fn(*a, **k)
        return f
    for name in NAMES:
        monkeypatch.setattr(CT, name, wrap(name, getattr(CT, name)))
    return counts


def test_every_layer_of_the_route_reaches_its_function(monkeypatch):
    m, x = network()
    counts = spy(monkeypatch)
    with V.vqvae_train("hip"):
        out, diff = m(x)
    assert counts == dict(stem_train=1, conv4x4s2_train=2, conv3x3_relu_train=4, res_block_train=8, conv1x1_relu_train=2, conv1x1_train=1,
                          convt4x4s2_train=3, head_train=1), counts
    assert type(out.grad_fn).__name__ == "_HeadBackward" and out.shape == x.shape and diff.shape == (1,)
    for name in NAMES:
        counts[name] = 0
    with V.vqvae_train("torch"):
        m(x)
    with V.vqvae_train("hip"), torch.no_grad():
        m(x)
    with V.vqvae_train("hip"), f16x3.decoder_conv("fp32"):
        m(x)
    assert not any(counts.values()), counts


def test_the_forward_is_the_fast_paths_bit_for_bit():
    m, x = network()
    fast = V._FastPath(copy.deepcopy(m).eval(), torch.device(DEV))
    q = torch.randn(2, 16, 16, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        lat0, img0 = fast.encode_latent(m, x), fast.decode(m, q)
    assert same_bits(CT.encode_latent_train(m, x).detach().permute(0, 2, 3, 1), lat0)
    assert same_bits(CT.decode_train(m, q.permute(0, 3, 1, 2)).detach(), img0)


def record(monkeypatch, masks):
    """The ReLU decisions of a run of the route, in the order the twins of tests/_vq_conv_train_ref.py meet them"""
    orig = {name: getattr(CT, name) for name in NAMES}

    def conv(name):
        def f(x, w, b, relu_in, *a, **k):
            if relu_in:
                xs = x.detach()
                masks.append(((V._d2s(xs, xs.size(1) // 4) if k.get("x_is_s2d") else xs) > 0).cpu())
            return orig[name](x, w, b, relu_in, *a, **k)
        return f

    def res(x, w3, b3, w1, b1, **k):
        xs = x.detach()
        h = f16x3.conv3x3(xs, f16x3.pack3x3(w3.detach(), b3.detach(), check=False), *f16x3.plain_relu(xs.size(0), xs.size(1), xs.device))
        masks.extend([(xs > 0).cpu(), (h[:, :w3.size(0)] > 0).cpu()])
        return orig["res_block_train"](x, w3, b3, w1, b1, **k)

    def first_relu(name):
        def f(x, *a, **k):
            masks.append((x.detach() > 0).cpu())
            return orig[name](x, *a, **k)
        return f
    for name in ("conv3x3_relu_train", "conv4x4s2_train", "convt4x4s2_train"):
        monkeypatch.setattr(CT, name, conv(name))
    monkeypatch.setattr(CT, "res_block_train", res)
    for name in ("conv1x1_relu_train", "head_train"):
        monkeypatch.setattr(CT, name, first_relu(name))


def against_the_twins(name, params, got, twin, loss_of, extra=()):
    """got: the route's gradients to params + extra; twin(P, mk, dtype) -> the twin's output; rule 2 per tensor, E32 torch's fp32 on the host"""
    grads = []
    for dtype in (D, torch.float32):
        P = ref.twin_params(params, dtype)
        more = [t.detach().cpu().to(dtype).clone().requires_grad_() for t in extra]
        mk = twin(P, more, dtype)
        grads.append(torch.autograd.grad(loss_of(mk[0], dtype), [P[id(p)] for p in params] + more))
        if dtype == D:
            mk = mk[1]
            print(f"{name}: {mk.flipped} of {mk.total} ReLU decisions differ from the twin's own signs; {mk.near} pre-activations within "
                  f"1e-4 max |.| of zero ({mk.near / mk.total:.2e})")
            assert mk.near <= 1e-3 * mk.total, "the condition of the test: choose another seed"
    ratios = [ref.rule2(f"{name} gradient {i} {tuple(a.shape)}", y, a, c, hold=False) for i, (y, a, c) in enumerate(zip(got, *grads))]
    assert max(ratios) <= 1.0, [(i, round(r, 3)) for i, r in enumerate(ratios) if r > 1.0]


def test_the_encoders_gradients_against_the_fp64_twin(monkeypatch):
    m, x = network()
    masks = []
    record(monkeypatch, masks)
    R = torch.randn(2, 64, 16, 16, generator=torch.Generator().manual_seed(6))
    params = ref.encoder_params(m)
    got = torch.autograd.grad((CT.encode_latent_train(m, x, CT.scale_for(m, x)) * R.to(DEV)).sum(), params)
    assert len(masks) == 13

    def twin(P, more, dtype):
        mk = ref.Masks(masks)
        return ref.encoder_twin(m, P, x.cpu().to(dtype), mk, dtype == D), mk
    against_the_twins("encoder", params, got, twin, lambda lat, dtype: (lat * R.to(dtype)).sum())


def test_the_decoders_gradients_against_the_fp64_twin(monkeypatch):
    m, x = network()
    masks = []
    record(monkeypatch, masks)
    gen = torch.Generator().manual_seed(7)
    q = torch.randn(2, 16, 16, 64, generator=gen).to(DEV).permute(0, 3, 1, 2).requires_grad_()
    target = torch.rand(2, 3, 128, 128, generator=gen)
    params = ref.decoder_params(m)
    got = torch.autograd.grad(F.mse_loss(CT.decode_train(m, q, CT.scale_for(m, x)), target.to(DEV)), params + [q])
    assert len(masks) == 6

    def twin(P, more, dtype):
        mk = ref.Masks(masks)
        return ref.decoder_twin(m, P, more[0], mk, dtype == D), mk
    against_the_twins("decoder", params, got, twin, lambda img, dtype: F.mse_loss(img, target.to(dtype)), extra=[q])


def test_one_train_step_and_twenty():
    m, x = network()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    before = {n: b.clone() for n, b in m.named_buffers()}
    with V.vqvae_train("hip"):
        assert type(m(x)[0].grad_fn).__name__ == "_HeadBackward"          # (the route is taken; this call's EMA update is part of `before`'s past)
        before = {n: b.clone() for n, b in m.named_buffers()}
        losses = [vq_train.train_step(m, opt, x)]
        assert all(v == v and abs(v) < float("inf") for v in losses[0])
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
        for q in ("quantize_t", "quantize_b"):
            for b in ("embed", "cluster_size", "embed_avg"):
                assert not torch.equal(before[f"{q}.{b}"], getattr(getattr(m, q), b)), (q, b)
        losses += [vq_train.train_step(m, opt, x) for _ in range(19)]
    print(f"reconstruction loss: {losses[0][0]:.6f} at step 1, {losses[-1][0]:.6f} at step 20")
    assert losses[-1][0] < losses[0][0]


def test_an_overflow_raises_before_the_optimiser_steps():
    m, x = network()
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    x = x.clone()
    x[0, :, 64:68, 64:68] = 1.0e6          # the stem (fp32) turns this into activations of 1e5 and more for the split-fp16 layer behind it
    before = [p.detach().clone() for p in m.parameters()]
    with V.vqvae_train("hip"):
        with pytest.raises(RuntimeError, match="beyond fp16's range"):
            vq_train.train_step(m, opt, x)
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
    f16x3.check_f16x3_overflow(torch.device(DEV))          # (the flag was cleared by the raise)
