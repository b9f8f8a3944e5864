"""GPU: the VGG19 content loss on the HIP kernels (csrc/content_loss.hip behind include/pixelsynth_content.h, losses/synthesis.py).

Operator level: the kernels through _lib.call against torch's device autograd of relu -> (max_pool2d) and l1_loss in fp32 on the same
tensors -- the pool and the join bit for bit (NaN positions included), the tap and the finish against the fp64 sum -- on the smallest
shapes at which the indexing can go wrong, with the values that decide something planted (zeros, a window whose maximum is 0, a window of
negatives, a positive tie, a NaN, a -inf).  Network level, 256 x 256, rand-init VGG19 with non-zero biases: the loss against the fp64
network, the gradient against the backward chain with the call's own decisions frozen (tests/_content_loss_ref.py derives both
bounds), its direction against torch's fp64 autograd, the routes and layouts, the overflow guard, ten Adam steps.  Every check prints its
error / bound.

Measured on the MI355X: pool and join bit for bit with torch's autograd in every case (at P = 3, where torch is allowed one ulp of c, it had the formula's bits too);
tap |L - L64| / L64 <= 1e-12; levels and total at most 0.14 of their bound; the frozen-chain gradient 0.73 (P = 1) and 0.71 (P = 2) of
its bound; cosine with fp64 autograd 0.99999 (torch fp32's 0.99998 / 0.99999); Total Loss 0.946 -> 0.779 over ten Adam steps.
"""
import types
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _content_loss_ref as ref
from pixelsynth_amd import _lib
from pixelsynth_amd.losses import synthesis as S
from pixelsynth_amd.networks import f16x3
from pixelsynth_amd.networks.vgg19 import VGG19

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
# (P, Hl, Wl, C): a single window; ragged tiles with P no power of two; the widest map; one more for the pool between / no pool pair
SHAPES = [(1, 2, 2, 64), (3, 6, 10, 64), (2, 32, 32, 512), (1, 16, 16, 128)]


def _maps(shape, seed, nan=True):
    """y (2P, C, Hl, Wl) channels_last with the deciding values planted in the prediction's first window(s) and in its target"""
    P, Hl, Wl, C = shape
    gen = torch.Generator().manual_seed(seed)
    y = torch.randn(2 * P, C, Hl, Wl, generator=gen)
    y[0, 0, :2, :2] = torch.tensor([[0.0, -1.0], [-2.0, -0.5]])          # a window whose maximum is 0 beside negatives
    y[0, 1, :2, :2] = torch.tensor([[-3.0, -1.0], [-2.0, -0.5]])         # a window of negatives
    y[0, 2, :2, :2] = torch.tensor([[0.25, 1.5], [1.5, -0.5]])           # a positive tie: the first one is torch's pick
    y[0, 3, :2, :2] = torch.tensor([[1.0, float("-inf")], [0.5, 2.0]])   # -inf is a negative value like any other
    y[0, 4, :2, :2] = 0.0                                                # exact zeros
    y[0, 5, :2, :2] = torch.tensor([[0.5, 0.5], [0.5, 0.5]])
    y[P, 5, :2, :2] = torch.tensor([[0.5, 0.75], [0.25, float("-inf")]])  # sign 0, -1, +1, +1 against the target
    y[P, 6, 0, 0] = float("-inf")
    if nan:
        y[0, 7, 0, 1] = float("nan")                                     # a NaN: picked by the pool, let through by the mask
        y[0, 8, 1, 1] = float("nan")
        y[0, 8, 0, 0] = 3.0
    return y.to(DEV).contiguous(memory_format=CL)


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_input_pass_reads_any_strides_and_changes_no_value():
    P, H, W = 2, 3, 5
    gen = torch.Generator().manual_seed(0)
    pred, gt = torch.randn(P, 3, H, W, generator=gen).to(DEV), torch.randn(P, 3, H, W, generator=gen).to(DEV)
    pred[0, 1, 2, 3], gt[1, 2, 0, 0] = float("nan"), float("-inf")
    big = torch.zeros(P + 1, 5, H + 2, 2 * W, device=DEV)
    big[1:, 1:4, 1:H + 1, ::2] = pred
    want = torch.zeros(2 * P, H, W, 4, device=DEV)
    want[:P, ..., :3], want[P:, ..., :3] = pred.permute(0, 2, 3, 1), gt.permute(0, 2, 3, 1)
    for a, b in ((pred, gt), (pred.contiguous(memory_format=CL), gt), (big[1:, 1:4, 1:H + 1, ::2], gt.contiguous(memory_format=CL))):
        out = torch.full((2 * P, H, W, 4), 7.0, device=DEV)
        _lib.call("ps_content_input", a, S._images.strides(a), b, S._images.strides(b), P, H, W, out)
        assert ref.same_bits(out, want)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_pool_is_max_pool2d_bit_for_bit(shape):
    P, Hl, Wl, C = shape
    y = _maps(shape, 1)
    b = torch.linspace(-0.5, 0.5, C, device=DEV)
    yb = y.clone(memory_format=CL)
    _lib.call("ps_content_bias", yb, b, 2 * P * Hl * Wl, C)              # the level-1 bias, added once
    assert ref.same_bits(yb, y + b.view(1, C, 1, 1)) and not ref.same_bits(yb, y)
    for src in (y, yb):
        out = torch.full((2 * P, C, Hl // 2, Wl // 2), 7.0, device=DEV).contiguous(memory_format=CL)
        _lib.call("ps_content_pool", src, 2 * P, Hl, Wl, C, out)
        want = F.max_pool2d(src, 2, 2)
        assert ref.same_bits(out, want) and bool(torch.isnan(out[0, 7, 0, 0])) and bool(torch.isnan(out[0, 8, 0, 0]))
        assert ref.same_bits(F.relu(out), F.max_pool2d(F.relu(src), 2, 2))          # the ReLU commutes with it
    print(f"pool {shape}: bit for bit")


def _tap_finish(y, P, level):
    _, C, Hl, Wl = y.shape
    tiles = _lib.call("ps_content_tiles", P * Hl * Wl)
    sums = torch.full((tiles + 1,), -7.0, dtype=torch.float64, device=DEV)
    _lib.call("ps_content_tap", y, P, Hl, Wl, C, sums)
    assert sums[tiles].item() == -7.0                                     # writes its tiles and nothing else
    t5, c5 = [0] * 5, [0] * 5
    t5[level], c5[level] = tiles, P * C * Hl * Wl
    levels = torch.full((5,), 7.0, device=DEV)
    total = torch.full((1,), 7.0, device=DEV)
    i64x5 = S.ctypes.c_int64 * 5
    _lib.call("ps_content_finish", sums, i64x5(*t5), i64x5(*c5), levels, total)
    return sums[:tiles].clone(), levels, total


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_tap_and_finish_against_the_fp64_sum(shape):
    P, Hl, Wl, C = shape
    y = _maps(shape, 2, nan=False)
    level = SHAPES.index(shape)
    sums, levels, total = _tap_finish(y, P, level)
    r = F.relu(y).double()
    N = P * C * Hl * Wl
    L64 = ((r[:P] - r[P:]).abs().sum() / N).item()
    s = 0.0
    for v in sums.tolist():                                               # the finish's one chain, ascending
        s += v
    L = s / N
    print(f"tap {shape}: |L - L64| / L64 = {abs(L - L64) / L64:.3e} / 1e-12")
    assert abs(L - L64) <= 1e-12 * L64
    want = [0.0] * 5
    want[level] = np.float32(L)
    assert levels.tolist() == [float(v) for v in want] and total.item() == float(np.float32(ref.WEIGHTS[level] * L))
    # the tiles: tile t is the prediction's pixels 256 t .. in (image, row, column) order
    per_pixel = (r[:P] - r[P:]).abs().sum(1).reshape(-1)
    for t in {0, len(sums) - 1}:
        want_t = per_pixel[256 * t:256 * (t + 1)].sum().item()
        assert abs(sums[t].item() - want_t) <= 1e-12 * max(want_t, 1e-300)
    again = _tap_finish(y, P, level)
    assert all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else _bits(a), b.view(torch.int64) if b.dtype == torch.float64 else _bits(b))
               for a, b in zip((sums, levels, total), again))
    nan_levels = _tap_finish(_maps(shape, 2), P, level)[1]
    assert bool(torch.isnan(nan_levels[level])) and float(nan_levels[(level + 1) % 5]) == 0.0      # a NaN stays one


JOINS = [(shape, pooled) for shape in SHAPES[:3] for pooled in (False, True)] + [(SHAPES[3], True), (SHAPES[3], False)]


@pytest.mark.parametrize("shape,pooled", JOINS, ids=str)
@pytest.mark.parametrize("inv_s,g", [(2.0 ** -20, 0.37), (1.0, 1.0), (2.0 ** 9, -2.5)], ids=str)
def test_join_is_torchs_backward_bit_for_bit(shape, pooled, inv_s, g):
    P, Hl, Wl, C = shape
    weight = 0.125
    both = _maps(shape, 3)
    y, y_gt = both[:P], both[P:]
    gen = torch.Generator().manual_seed(4)
    up_shape = (P, C, Hl // 2, Wl // 2) if pooled else (P, C, Hl, Wl)
    up = (torch.randn(up_shape, generator=gen) / inv_s).to(DEV).contiguous(memory_format=CL)    # still multiplied by its scale
    scale2 = torch.tensor([1.0 / inv_s, inv_s], device=DEV)
    g_dev = torch.tensor([g], device=DEV)
    N = P * C * Hl * Wl
    c = ref.seed_c(g, weight, N)

    def run(y_gt_, up_):
        G = torch.full_like(y, 7.0)
        _lib.call("ps_content_join", y, y_gt_, up_, None if up_ is None else scale2, None if y_gt_ is None else g_dev, weight, P, Hl, Wl, C,
                  int(pooled and up_ is not None), G)
        return G

    def autograd(y_gt_, up_):
        leaf = y.clone(memory_format=CL).requires_grad_()
        r = F.relu(leaf)
        outs, grads = [], []
        if up_ is not None:
            outs.append(((F.max_pool2d(r, 2, 2) if pooled else r) * (up_ * inv_s)).sum())
            grads.append(torch.ones((), device=DEV))
        if y_gt_ is not None:
            outs.append(weight * F.l1_loss(r, F.relu(y_gt_)))
            grads.append(g_dev[0])
        torch.autograd.backward(outs, grads)
        return leaf.grad

    cases = [("up + seed", y_gt, up), ("up alone", None, up)] + ([] if pooled else [("seed alone (up = NULL)", y_gt, None)])
    for name, y_gt_, up_ in cases:
        G = run(y_gt_, up_)
        want = ref.join_formula(y, y_gt_, up_, inv_s, c, pooled)
        torchs = autograd(y_gt_, up_)
        assert ref.same_bits(G, want), name
        assert bool((G[0, :2, :2, :2] == 0).all()) and bool((G[0, 4, :2, :2] == 0).all())          # nothing through y <= 0
        assert bool((torch.isnan(G) == torch.isnan(torchs)).all())
        diff = (G - torchs).abs().nan_to_num(0.0).max().item()
        ulp = float(np.spacing(np.float32(abs(c)))) if y_gt_ is not None else 0.0
        print(f"join {shape} pooled {pooled} inv_s {inv_s:g} g {g:g} {name}: formula bit for bit; against torch's autograd {diff:.3e} / {ulp:.3e}")
        if P != 3:
            assert ref.same_bits(G, torchs), name
        else:       # N is no power of two: torch may form c as (g w) * (1 / N), so it is allowed one ulp of c (measured: the same bits)
            assert diff <= ulp, name
        assert ref.same_bits(G, run(y_gt_, up_)), name                    # two runs, the same bits


# ---- network level ------------------------------------------------------------------------------------------------------------------------------
_NET = {}


def _vgg(seed=10):
    torch.manual_seed(seed)
    vgg = VGG19(rand=True)
    with torch.no_grad():
        for conv in vgg.convs():
            conv.bias.normal_(0.0, 0.1)
    return vgg.to(DEV)


def _images(P, size=256, seed=11):
    gen = torch.Generator().manual_seed(seed + P)
    return torch.tanh(torch.randn(P, 3, size, size, generator=gen)).to(DEV), torch.tanh(torch.randn(P, 3, size, size, generator=gen)).to(DEV)


def _case(P):
    """One HIP call with its saved maps, torch's fp32 modules and the fp64 network on the same inputs: computed once per P"""
    if P not in _NET:
        vgg = _vgg()
        pred, gt = _images(P)
        leaf = pred.clone().requires_grad_()
        assert S.hip_takes(vgg, leaf, gt)
        total, levels, saved = S.content_loss(vgg, leaf, gt, return_saved=True)
        grad, = torch.autograd.grad(total, leaf)
        sd = vgg.state_dict()
        leaf32 = pred.clone().requires_grad_()
        with f16x3.decoder_conv("fp32"):
            total32, levels32 = S.content_loss(vgg, leaf32, gt)
        grad32, = torch.autograd.grad(total32, leaf32)
        leaf64 = pred.double().requires_grad_()
        total64, levels64 = ref.loss(ref.cast(sd, torch.float64), leaf64, gt.double())
        grad64, = torch.autograd.grad(total64, leaf64)
        torch.cuda.synchronize()
        _NET[P] = types.SimpleNamespace(vgg=vgg, sd=sd, pred=pred, gt=gt, total=total.detach(), levels=levels, saved=saved, grad=grad,
                                        total32=total32.detach(), levels32=levels32, grad32=grad32, total64=total64.detach(),
                                        levels64=torch.stack(levels64).detach(), grad64=grad64)
    return _NET[P]


@pytest.mark.parametrize("P", [1, 2])
def test_loss_values_against_the_fp64_network(P):
    n = _case(P)
    assert n.total.dtype == torch.float32 and n.total.dim() == 0 and n.levels.shape == (5,) and not n.levels.requires_grad
    for l in range(5):
        err, bound = ref.rule(f"P {P} level {l + 1}", n.levels[l], n.levels64[l], n.levels32[l])
        assert err <= bound
    err, bound = ref.rule(f"P {P} total", n.total, n.total64, n.total32)
    assert err <= bound


@pytest.mark.parametrize("P", [1, 2])
def test_gradient_against_the_frozen_mask_chain(P):
    n = _case(P)
    maps, gts = n.saved["maps"], n.saved["gt"]
    assert [tuple(m.shape) for m in maps] == [(P, C, 256 >> l, 256 >> l) for C, l in zip(ref.WIDTHS, (0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4))]
    assert [tuple(m.shape) for m in gts] == [tuple(maps[k].shape) for k in ref.TAPPED]
    assert n.grad.shape == n.pred.shape and bool(torch.isfinite(n.grad).all())
    g64 = ref.frozen_chain(n.sd, n.saved, 1.0, torch.float64)
    g32 = ref.frozen_chain(n.sd, n.saved, 1.0, torch.float32)
    err, bound = ref.rule(f"P {P} gradient, frozen chain", n.grad, g64, g32)
    assert err <= bound


@pytest.mark.parametrize("P", [1, 2])
def test_gradient_direction_against_torchs_fp64_autograd(P):
    n = _case(P)
    cos = lambda a, b: F.cosine_similarity(a.double().reshape(1, -1), b.double().reshape(1, -1)).item()
    ours, torchs = cos(n.grad, n.grad64), cos(n.grad32, n.grad64)
    print(f"P {P} free-running gradient against fp64 autograd: cosine {ours:.6f} (>= 0.99); torch fp32's {torchs:.6f}")
    assert ours >= 0.99


def test_routes_and_layouts():
    n = _case(2)
    vgg, pred, gt = n.vgg, n.pred, n.gt
    big = torch.zeros(3, 4, 258, 512, device=DEV)
    big[1:, :3, 1:257, ::2] = pred
    for name, p in (("channels_last", pred.contiguous(memory_format=CL)), ("a strided view", big[1:, :3, 1:257, ::2])):
        leaf = p.detach().requires_grad_()
        total, levels = S.content_loss(vgg, leaf, gt.contiguous(memory_format=CL) if name == "channels_last" else gt)
        grad, = torch.autograd.grad(total, leaf)
        assert ref.same_bits(total, n.total) and ref.same_bits(levels, n.levels) and ref.same_bits(grad, n.grad), name
    # no grad: nothing saved, the same total
    leaf = pred.clone().requires_grad_()
    with torch.no_grad():                                                     # (a prediction that requires grad: grad mode decides)
        total, levels, saved = S.content_loss(vgg, leaf, gt, return_saved=True)
    assert saved is None and ref.same_bits(total, n.total) and not total.requires_grad
    total, _, saved = S.content_loss(vgg, pred, gt, return_saved=True)        # (nothing requires grad)
    assert saved is None and ref.same_bits(total, n.total)
    # the torch route: another size, the switch, a target that requires grad
    small_p, small_g = _images(2, 128)
    for name, p, g, ctx in (("128 x 128", small_p, small_g, None), ("decoder_conv fp32", pred, gt, f16x3.decoder_conv("fp32")),
                            ("gt requires grad", pred, gt.clone().requires_grad_(), None)):
        leaf = p.clone().requires_grad_()
        assert ctx is not None or not S.hip_takes(vgg, leaf, g), name
        if ctx is None:
            total, levels, saved = S.content_loss(vgg, leaf, g, return_saved=True)
        else:
            with ctx:
                assert not S.hip_takes(vgg, leaf, g)
                total, levels, saved = S.content_loss(vgg, leaf, g, return_saved=True)
        want, want_levels = S.torch_content_loss(vgg, leaf, g)
        assert saved is None and total.requires_grad
        rel = abs(total.item() - want.item()) / want.item()
        print(f"torch route, {name}: against torch_content_loss {rel:.3e} / 1e-6")
        assert rel <= 1e-6 and torch.allclose(levels, want_levels, rtol=1e-6, atol=0)
        if name == "gt requires grad":
            ggt, = torch.autograd.grad(total, g)
            assert float(ggt.abs().max()) > 0


def test_an_overflow_warns_and_returns_the_torch_routes_value():
    vgg = _vgg()
    with torch.no_grad():
        vgg.convs()[1].weight.mul_(1.0e5)                                     # conv1_2's output leaves fp16's range
    pred, gt = _images(1)
    leaf = pred.clone().requires_grad_()
    assert S.hip_takes(vgg, leaf, gt)
    with pytest.warns(UserWarning, match="fp16's range"):
        total, levels, saved = S.content_loss(vgg, leaf, gt, return_saved=True)
    want, _ = S.torch_content_loss(vgg, leaf, gt)
    rel = abs(total.item() - want.item()) / want.item()
    print(f"overflow: total {total.item():.6e} against the torch route's {want.item():.6e}: {rel:.3e} / 1e-6")
    assert saved is None and rel <= 1e-6
    grad, = torch.autograd.grad(total, leaf)
    assert bool(torch.isfinite(grad).all())
    with warnings.catch_warnings():                                          # and the flag is left clear
        warnings.filterwarnings("error", message=".*fp16's range.*")
        S.content_loss(_case(1).vgg, pred, gt)


def test_ten_adam_steps_under_synthesis_loss():
    torch.manual_seed(20)
    crit = S.SynthesisLoss(types.SimpleNamespace(losses=["1.0_l1", "10.0_content"], vgg19_rand=True)).to(DEV)
    _, gt = _images(1)
    param = torch.randn(1, 3, 256, 256, device=DEV).requires_grad_()
    opt = torch.optim.Adam([param], lr=0.05)
    values = []
    for _ in range(10):
        pred = torch.tanh(param)
        assert S.hip_takes(crit.losses[1].model, pred, gt)
        out = crit(pred, gt)
        opt.zero_grad()
        out["Total Loss"].backward()
        opt.step()
        values.append(out["Total Loss"].item())
    print("Total Loss over ten Adam steps:", " ".join(f"{v:.5f}" for v in values))
    assert values[-1] < values[0] and all(np.isfinite(values))
    assert set(out) == {"L1", "Perceptual", "Total Loss", "psnr", "ssim"}
    with torch.no_grad():
        mse = (pred - gt).pow(2).sum(1).view(1, -1).mean(1)
        psnr = (10 * (1 / mse).log10()).mean()
        want_ssim = S._ssim_host(pred.double().cpu(), gt.double().cpu()).item()
    print(f"psnr {out['psnr'].item():.6f} against {psnr.item():.6f}; ssim {out['ssim'].item():.7f} against fp64 {want_ssim:.7f}: "
          f"{abs(out['ssim'].item() - want_ssim):.3e} / 1e-5")
    assert torch.equal(out["psnr"], psnr) and not out["ssim"].requires_grad
    # (ten times the 1e-6 the metric kernel's own tests allow on pairs that are not flat: these images span twice the range)
    assert abs(out["ssim"].item() - want_ssim) <= 1e-5
