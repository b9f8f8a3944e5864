"""GPU: the backward pass of the locally masked convolution (csrc/lmconv_bwd.hip behind include/pixelsynth_lmconv_bwd.h, the autograd
Function of lmconv/locally_masked_convolution.py, likelihood.ar_loss).

Operator level: every gradient against fp64 torch autograd of the oracle's unfold formula on the same fp32 inputs, inside the DERIVED
rounding bounds of tests/_lmconv_bwd_ref.py (its docstring says where they come from); exact zeros where every term is closed.

Network level (PixelSynth's OurPixelCNN, an 8 x 8 grid, two frames with random orders, the second half of each order sampled):
ar_loss against the fused engine's score, every parameter gradient against the fp64 twin (oracle.lmconv_oracle.pixelcnn_forward in
fp64 on the CPU) with the same twin in fp32 as the yardstick, and ten Adam steps that the rebuilt engine has to see.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _lmconv_bwd_ref as ref
from oracle import c_oracle, lmconv_oracle as lo
from pixelsynth_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(B, Ci, Co, H, W, Bm, frac, seed=0, bias=True):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Ci, H, W, generator=gen)
    w = torch.randn(Co, Ci, 3, 3, generator=gen) * 0.1
    b = torch.randn(Co, generator=gen) if bias else None
    m = torch.rand(Bm, 9, H * W, generator=gen)
    m = torch.where(m < 0.4, torch.zeros_like(m), m if frac else torch.ones_like(m))
    g = torch.randn(B, Co, H, W, generator=gen)
    return x, m, w, b, g


def _hip_gradients(x, m, w, b, g, dil):
    """Through the module's Function on the device -> (y, grad_x, grad_w, grad_bias or None)"""
    from pixelsynth_amd.lmconv.locally_masked_convolution import _locally_masked_conv2d
    dx, dw = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    db = None if b is None else b.to(DEV).requires_grad_()
    y = _locally_masked_conv2d.apply(dx, m.to(DEV), dw, None, db, dil, dil)
    assert y.requires_grad and y.grad_fn is not None
    y.backward(g.to(DEV))
    torch.cuda.synchronize()
    return y.detach(), dx.grad, dw.grad, None if b is None else db.grad


def _check_case(name, x, m, w, b, g, dil):
    want = ref.gradients(x, m, w, b, g, dil)
    bound = ref.bounds(x, m, w, g, dil)
    _, gx, gw, gb = _hip_gradients(x, m, w, b, g, dil)
    assert gx.shape == x.shape and gw.shape == w.shape and gx.dtype == gw.dtype == torch.float32
    ref.check(f"{name} grad_x", gx, want[0], bound[0])
    ref.check(f"{name} grad_w", gw, want[1], bound[1])
    if b is not None:
        assert gb.shape == b.shape
        ref.check(f"{name} grad_bias", gb, want[2], bound[2])


def test_broadcast_mask_dilation_2_no_bias_locations_no_multiple_of_4():
    x, m, w, b, g = _inputs(3, 7, 5, 6, 9, 1, False, bias=False)
    assert (3 * 6 * 9) % 4 != 0
    _check_case("B3 7->5 6x9 d2", x, m, w, b, g, 2)


def test_per_image_fractional_masks_with_zeros_and_bias():
    x, m, w, b, g = _inputs(2, 7, 5, 6, 9, 2, True, seed=1)
    assert (m == 0).any() and ((m > 0) & (m < 1)).any()
    m[:, :, 7] = 0                                       # a location with every tap closed: its terms are exact zeros
    m[1, 3] = 0                                          # a tap closed everywhere in one image
    _check_case("B2 7->5 6x9 d1 fractional", x, m, w, b, g, 1)
    # every tap closed everywhere: every gradient but the bias' is exactly 0
    _, gx, gw, gb = _hip_gradients(x, torch.zeros_like(m), w, b, g, 1)
    assert not gx.any() and not gw.any() and gb.abs().max() > 0


@pytest.mark.parametrize("Ci,Co,dil", [(160, 80, 1), (160, 160, 1), (80, 80, 2)])
def test_the_network_layer_shapes(Ci, Co, dil):
    x, m, w, b, g = _inputs(2, Ci, Co, 8, 8, 2, Ci == 80, seed=Ci + Co)
    _check_case(f"B2 {Ci}->{Co} 8x8 d{dil}", x, m, w, b, g, dil)


def test_the_input_layer_with_the_mask_in_the_repeated_form():
    B, Ci, Co, H, W = 1, 513, 80, 8, 8
    x, m, w, b, g = _inputs(B, Ci, Co, H, W, 1, False, seed=5)
    rep = m.unsqueeze(1).repeat(1, Ci, 1, 1).reshape(B * Ci, 9, H * W)
    _check_case("B1 513->80 8x8 repeated mask", x, rep, w, b, g, 1)
    a, c = _hip_gradients(x, rep, w, b, g, 1), _hip_gradients(x, m, w, b, g, 1)
    assert all(torch.equal(p, q) for p, q in zip(a, c))


def test_a_reduction_that_spans_several_parts():
    x, m, w, b, g = _inputs(5, 16, 16, 32, 32, 5, True, seed=7)
    _check_case("B5 16->16 32x32", x, m, w, b, g, 1)


def test_sum_backward_and_a_sliced_grad_output():
    from pixelsynth_amd.lmconv.locally_masked_convolution import _locally_masked_conv2d
    x, m, w, b, g = _inputs(2, 7, 5, 6, 9, 2, True, seed=3)
    dx, dw, db = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    _locally_masked_conv2d.apply(dx, m.to(DEV), dw, None, db, 2, 2).sum().backward()       # (grad_output: a stride-0 expansion)
    ones = torch.ones_like(g)
    want, bound = ref.gradients(x, m, w, b, ones, 2), ref.bounds(x, m, w, ones, 2)
    for name, got, k in (("grad_x", dx.grad, 0), ("grad_w", dw.grad, 1), ("grad_bias", db.grad, 2)):
        ref.check(f"sum().backward() {name}", got, want[k], bound[k])
    assert torch.equal(db.grad.cpu(), torch.full((5,), 2.0 * 6 * 9))
    # a non-contiguous grad_output: every second channel of a wider tensor
    wide = torch.randn(2, 10, 6, 9, generator=torch.Generator().manual_seed(4))
    sliced = wide.to(DEV)[:, ::2]
    assert not sliced.is_contiguous()
    for t in (dx, dw, db):
        t.grad = None
    _locally_masked_conv2d.apply(dx, m.to(DEV), dw, None, db, 2, 2).backward(sliced)
    g2 = wide[:, ::2].contiguous()
    want, bound = ref.gradients(x, m, w, b, g2, 2), ref.bounds(x, m, w, g2, 2)
    for name, got, k in (("grad_x", dx.grad, 0), ("grad_w", dw.grad, 1), ("grad_bias", db.grad, 2)):
        ref.check(f"sliced grad_output {name}", got, want[k], bound[k])


@pytest.mark.parametrize("which", ["x", "weight", "bias"])
def test_only_what_requires_grad_gets_one(which):
    from pixelsynth_amd.lmconv.locally_masked_convolution import locally_masked_conv2d
    x, m, w, b, g = _inputs(2, 7, 5, 6, 9, 2, True, seed=3)
    layer = locally_masked_conv2d(7, 5, dilation=2).to(DEV)
    with torch.no_grad():
        layer.weight.copy_(w)
        layer.bias.copy_(b)
    layer.weight.requires_grad_(which == "weight")
    layer.bias.requires_grad_(which == "bias")
    dx = x.to(DEV).requires_grad_(which == "x")
    layer(dx, m.to(DEV)).backward(g.to(DEV))
    got = {"x": dx.grad, "weight": layer.weight.grad, "bias": layer.bias.grad}
    assert [k for k, v in got.items() if v is not None] == [which]
    k = ("x", "weight", "bias").index(which)
    ref.check(f"alone grad_{which}", got[which], ref.gradients(x, m, w, b, g, 2)[k], ref.bounds(x, m, w, g, 2)[k])


def test_forward_bits_and_two_backward_runs():
    from pixelsynth_amd.lmconv.locally_masked_convolution import lmconv_forward
    x, m, w, b, g = _inputs(5, 16, 16, 32, 32, 5, True, seed=7)
    first = _hip_gradients(x, m, w, b, g, 1)
    with torch.no_grad():
        plain = lmconv_forward(x.to(DEV), m.to(DEV), w.to(DEV), b.to(DEV), 1)
    assert not plain.requires_grad and torch.equal(first[0], plain)
    again = _hip_gradients(x, m, w, b, g, 1)
    for name, p, q in zip(("y", "grad_x", "grad_w", "grad_bias"), first, again):
        assert torch.equal(p, q), name


# ---------------------------------------------------------------------------------------------------------------- network level
H8 = W8 = 8
L8, B8 = H8 * W8, 2
C_GRAD = 4         # e_k(HIP) <= C_GRAD * E: the smallest power of two at or above twice the largest ratio measured on the MI355X, 1.251
                   # (docs/LAB_NOTEBOOK.md section 9 has the five largest)
_NET = {}


def _setup():
    """Two random orders, their masks from the oracle, codes, the sampled region (the second half of each order); computed once"""
    if not _NET:
        rs = np.random.RandomState(0)
        orders = [np.stack(np.unravel_index(rs.permutation(L8), (H8, W8)), 1).astype(np.int32) for _ in range(B8)]
        masks = [np.concatenate([c_oracle.unfolded_masks(o, H8, W8, 3, dil, typ) for o in orders]) for dil, typ in ((1, "A"), (1, "B"), (2, "B"))]
        codes = rs.randint(0, 512, (B8, H8, W8)).astype(np.int64)
        region = np.zeros((B8, L8), np.uint8)
        for b, o in enumerate(orders):
            loc = o[:, 0] * W8 + o[:, 1]
            region[b, loc[L8 // 2:]] = 1
        _NET.update(masks=[torch.from_numpy(m) for m in masks], codes=torch.from_numpy(codes), region=torch.from_numpy(region))
    return _NET["masks"], _NET["codes"], _NET["region"]


def val(t):
    return float(t.detach())


def _net(seed=0):
    from test_lmconv_gpu import make_net
    return make_net(seed)


def _twin_gradients(dtype):
    """The oracle's network at `dtype` on the CPU -> (loss, {parameter name: gradient})"""
    masks, codes, region = _setup()
    sd = {k: torch.from_numpy(v).to(dtype).requires_grad_() for k, v in syn.pixelcnn_state_dict(0).items()}
    x = F.one_hot(codes, 512).permute(0, 3, 1, 2).to(dtype)
    logits = lo.pixelcnn_forward(sd, x, *[m.to(dtype) for m in masks]).reshape(B8, 512, L8)
    loss = F.cross_entropy(logits, codes.reshape(B8, L8), reduction="none")[region.bool()].mean()
    return float(loss.detach()), dict(zip(sd, torch.autograd.grad(loss, list(sd.values()))))


def test_ar_loss_is_the_engine_score():
    from pixelsynth_amd.likelihood import ar_loss, score_codes
    masks, codes, region = _setup()
    net = _net()
    dm, dc, dr = [m.to(DEV) for m in masks], codes.to(DEV), region.to(DEV)
    loss = ar_loss(net, dc, dm, region=dr)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad and loss.is_cuda
    with torch.no_grad():
        logits = net.engine(H8, W8, B8).forward(dc, *dm)
        score = score_codes(net, dc, dm, region=dr)
    tol = 2 * (1e-4 + 1e-4 * float(logits.abs().max()))
    print(f"ar_loss {val(loss):.6f}  engine mean_nll(sampled) {float(score.mean_nll('sampled')):.6f}  tolerance {tol:.2e}")
    assert abs(val(loss) - float(score.mean_nll("sampled"))) <= tol
    for group in ("all", "observed"):
        assert abs(val(ar_loss(net, dc, dm, region=dr, group=group)) - float(score.mean_nll(group))) <= tol, group
    # the reference's calling convention for the masks, and a temperature
    rep = [m.unsqueeze(1).repeat(1, c, 1, 1).reshape(B8 * c, 9, L8) for m, c in zip(dm, (513, 160, 80))]
    assert abs(val(ar_loss(net, dc, rep, region=dr)) - val(loss)) <= 1e-6 * val(loss)
    with torch.no_grad():
        cool = score_codes(net, dc, dm, region=dr, temperature=0.7)
    assert abs(val(ar_loss(net, dc, dm, region=dr, temperature=0.7)) - float(cool.mean_nll("sampled"))) <= tol / 0.7


def test_parameter_gradients_against_the_fp64_twin():
    from pixelsynth_amd.likelihood import ar_loss
    masks, codes, region = _setup()
    net = _net()
    loss = ar_loss(net, codes.to(DEV), [m.to(DEV) for m in masks], region=region.to(DEV))
    loss.backward()
    l64, g64 = _twin_gradients(torch.float64)
    l32, g32 = _twin_gradients(torch.float32)
    got = {k: p.grad for k, p in net.named_parameters()}
    assert set(got) == set(g64) and all(v is not None for v in got.values())
    err = lambda g, k: float((g[k].detach().cpu().double() - g64[k]).abs().max() / g64[k].abs().max())
    assert all(float(v.abs().max()) > 0 for v in g64.values())
    e_twin = {k: err(g32, k) for k in g64}
    e_hip = {k: err(got, k) for k in g64}
    E = max(e_twin.values())
    worst = max(e_hip, key=e_hip.get)
    print(f"loss: HIP {val(loss):.6f} twin fp32 {l32:.6f} fp64 {l64:.6f}")
    print(f"twin fp32: E = max e_k {E:.3e}, median {np.median(list(e_twin.values())):.3e}")
    print(f"HIP: max e_k {e_hip[worst]:.3e} ({worst}), median {np.median(list(e_hip.values())):.3e}; largest e_k(HIP) / E = {e_hip[worst] / E:.3f}")
    for k in sorted(e_hip, key=e_hip.get)[-5:]:
        print(f"    {k}: e_k(HIP) / E = {e_hip[k] / E:.3f}")
    assert all(e <= C_GRAD * E for e in e_hip.values()), (worst, e_hip[worst] / E)


def test_ten_adam_steps_reach_the_rebuilt_engine():
    from pixelsynth_amd.likelihood import ar_loss, score_codes
    masks, codes, region = _setup()
    net = _net()
    dm, dc, dr = [m.to(DEV) for m in masks], codes.to(DEV), region.to(DEV)
    with torch.no_grad():
        start = float(score_codes(net, dc, dm, region=dr).mean_nll("sampled"))
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    for _ in range(10):
        opt.zero_grad()
        ar_loss(net, dc, dm, region=dr).backward()
        opt.step()
    with torch.no_grad():
        end = float(score_codes(net, dc, dm, region=dr).mean_nll("sampled"))
    print(f"engine mean_nll(sampled): {start:.4f} before, {end:.4f} after ten Adam steps")
    assert end < 0.5 * start
