"""GPU: the training step's glue kernels (csrc/train_glue.hip behind include/pixelsynth_train_glue.h) through their autograd Functions
(networks/train_glue.py).

combine_mask_nhwc: forward and backward BIT FOR BIT against the torch formula on the device (get_combined, the mask channel, the
channels-last copy; autograd's own backward) -- on (B,H,W) = (1,1,1), (1,3,5), (2,8,64), (3,16,16) and one row of 255 / 256 / 257 pixels
(both sides of the 256-lane workgroup: a partial last workgroup, an exact one, one lane into the next); with NaN, +-inf and -0 planted in
either operand and in the gradient under both mask values; a frame alone against the same frame as frame 1 of 3; twice.

depth_head: both modes on 0.3 + 1.5 randn, on +-30 and on a 1 x 1 map inside the bound tests/_train_glue_ref.py derives; PredDepthImg bit
for bit depth / 5 - 1; the gradient under the project's rule with no element left out; the same batch-independence check."""
import pytest
import torch

import _train_glue_ref as ref
from pixelsynth_amd.networks import train_glue as tg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPECIALS = (float("nan"), float("inf"), float("-inf"), -0.0)


def operands(B, H, W, seed=0):
    gen = torch.Generator().manual_seed(seed)
    g, t = torch.randn(B, 3, H, W, generator=gen), torch.randn(B, 3, H, W, generator=gen)
    m = torch.rand(B, H, W, generator=gen) > 0.4
    dy = torch.randn(B, 4, H, W, generator=gen)
    return g, t, m, dy


def run_combine(route, g, t, m, dy):
    """-> (out as dense NCHW values, its strides, grad of gen_fs) on the device through `route`"""
    a = g.to(DEV).requires_grad_()
    with tg.train_glue(route):
        out = tg.combine_mask_nhwc(a, t.to(DEV), m.to(DEV))
    assert (type(out.grad_fn).__name__ == "CombineMaskNHWCBackward") == (route == "hip"), f"route {route}: {type(out.grad_fn).__name__}"
    out.backward(dy.to(DEV))
    return out.detach(), a.grad


def assert_combine_matches(g, t, m, dy, name):
    out_h, grad_h = run_combine("hip", g, t, m, dy)
    out_t, grad_t = run_combine("torch", g, t, m, dy)
    B, _, H, W = g.shape
    assert out_h.shape == (B, 4, H, W) and out_h.permute(0, 2, 3, 1).is_contiguous(), name     # what ResNetDecoder reads first
    assert ref.same_bits(out_h, out_t), f"{name}: forward"
    assert ref.same_bits(out_h, ref.combine_formula(g.to(DEV), t.to(DEV), m.to(DEV))), f"{name}: forward against the written-out formula"
    assert grad_h.shape == g.shape and grad_h.is_contiguous() and ref.same_bits(grad_h, grad_t), f"{name}: backward"
    return out_h, grad_h


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (1, 3, 5), (2, 8, 64), (3, 16, 16), (1, 1, 255), (1, 1, 256), (1, 1, 257)])
def test_combine_is_the_torch_formula_bit_for_bit(B, H, W):
    g, t, m, dy = operands(B, H, W, seed=B * H * W)
    if m.numel() > 2:
        m.view(-1)[0], m.view(-1)[-1] = True, False          # both values in every case that has room, the last pixel included
    out, grad = assert_combine_matches(g, t, m, dy, f"{B}x{H}x{W}")
    again = run_combine("hip", g, t, m, dy)
    assert ref.same_bits(out, again[0]) and ref.same_bits(grad, again[1]), "two runs differ"


def test_combine_keeps_nan_inf_and_negative_zero_as_the_formula_does():
    # pixel = (special value) x (which operand holds it: gen, gt, the gradient) x (mask value); the other operands are ordinary
    n = len(SPECIALS) * 3 * 2
    g, t, _, dy = operands(1, 1, n, seed=3)
    m = torch.zeros(1, 1, n, dtype=torch.bool)
    p = 0
    for v in SPECIALS:
        for holder in (g, t, dy):
            for bg in (False, True):
                holder[0, :3, 0, p] = v
                m[0, 0, p] = bg
                p += 1
    out, grad = assert_combine_matches(g, t, m, dy, "specials")
    # what the formula says of them, stated once so that the comparison above is not two wrongs agreeing
    o, gr = out.cpu(), grad.cpu()
    assert torch.isnan(o[0, 0, 0, 0]) and torch.isnan(o[0, 0, 0, 1])          # NaN in gen: NaN * 1 and NaN * 0
    assert torch.isnan(o[0, 0, 0, 2]) and torch.isnan(o[0, 0, 0, 3])          # NaN in gt: under both masks too
    assert torch.isnan(gr[0, 0, 0, 4]) and torch.isnan(gr[0, 0, 0, 5])        # a NaN gradient stays one where the mask is set
    assert o[0, 0, 0, 6] == float("inf") and torch.isnan(o[0, 0, 0, 7])       # +inf in gen: kept in the foreground, inf * 0 behind
    assert (o[0, 3, 0] == (~m[0, 0]).float()).all()


def test_combine_frame_does_not_depend_on_the_batch():
    g, t, m, dy = operands(3, 16, 24, seed=5)
    out3, grad3 = run_combine("hip", g, t, m, dy)
    out1, grad1 = run_combine("hip", g[1:2], t[1:2], m[1:2], dy[1:2])
    assert ref.same_bits(out3[1:2], out1) and ref.same_bits(grad3[1:2], grad1)


def test_combine_routes():
    g, t, m, _ = operands(2, 8, 8)
    gd, td, md = g.to(DEV), t.to(DEV), m.to(DEV)
    assert tg.combine_takes(gd, td, md)
    assert not tg.combine_takes(gd, td.requires_grad_(), md)                                  # input_gt wants a gradient: the formula's
    td = td.detach()
    assert not tg.combine_takes(gd.double(), td.double(), md) and not tg.combine_takes(gd[:, :2], td[:, :2], md)
    assert not tg.combine_takes(gd, td, md.to(torch.uint8)) and not tg.combine_takes(gd.transpose(2, 3), td.transpose(2, 3), md)
    with tg.train_glue("hip"):
        a, b = gd.clone().requires_grad_(), td.clone().requires_grad_()
        out = tg.combine_mask_nhwc(a, b, md)
        assert type(out.grad_fn).__name__ != "CombineMaskNHWCBackward"
        out.sum().backward()
        assert ref.same_bits(b.grad, md.float().unsqueeze(1).expand_as(b))
        with torch.no_grad():                                                                 # without grad mode the kernel still runs
            assert ref.same_bits(tg.combine_mask_nhwc(gd, td, md), out)


# ------------------------------------------------------------------------------------------------------------------ the depth head
def run_depth(raw, mode, dy):
    a = raw.to(DEV).requires_grad_()
    with tg.train_glue("hip"):
        depth, pred = tg.depth_head(a, mode, ref.MIN_Z, ref.MAX_Z)
    assert type(depth.grad_fn).__name__ == "DepthHeadBackward", "the HIP route was not taken"
    assert not pred.requires_grad
    depth.backward(dy.to(DEV))
    return depth.detach(), pred, a.grad


@pytest.mark.parametrize("mode", [ref.RANGE, ref.INVERSE])
@pytest.mark.parametrize("shape,kind", [((2, 1, 15, 17), "randn"), ((2, 1, 15, 17), "large"), ((1, 1, 1, 1), "randn"), ((3, 1, 16, 16), "randn")])
def test_depth_head_within_the_derived_bound(mode, shape, kind):
    raw = ref.raws(shape, kind, seed=len(kind) + shape[0])
    dy = torch.randn(shape, generator=torch.Generator().manual_seed(1))
    depth, pred, grad = run_depth(raw, mode, dy)
    name = f"mode {mode} {kind} {shape}"
    d64, bound = ref.depth_bound(raw, mode)
    assert ref.check(f"{name} depth", depth, d64, bound) <= 1.0
    assert ref.same_bits(pred, ref.pred_img_host(depth)), f"{name}: PredDepthImg is not depth / 5 - 1"
    fn = lambda a: ref.depth_formula(a, mode)
    (g64,), (g32,) = ref.autograd(fn, (raw,), dy, torch.float64), ref.autograd(fn, (raw,), dy, torch.float32)
    gbound, e32 = ref.grad_bound(g32, g64)
    print(f"{name}: E32 {e32:.3e}")
    assert ref.check(f"{name} grad", grad, g64, gbound) <= 1.0
    again = run_depth(raw, mode, dy)
    assert all(ref.same_bits(a, b) for a, b in zip((depth, pred, grad), again)), "two runs differ"


@pytest.mark.parametrize("mode", [ref.RANGE, ref.INVERSE])
def test_depth_head_frame_does_not_depend_on_the_batch(mode):
    raw = ref.raws((3, 1, 16, 24), "randn", seed=7)
    dy = torch.randn(raw.shape, generator=torch.Generator().manual_seed(2))
    three, one = run_depth(raw, mode, dy), run_depth(raw[1:2], mode, dy[1:2])
    assert all(ref.same_bits(a[1:2], b) for a, b in zip(three, one))


def test_depth_head_routes():
    raw = ref.raws((2, 1, 8, 8), "randn").to(DEV)
    assert tg.depth_takes(raw) and not tg.depth_takes(raw.double()) and not tg.depth_takes(raw.expand(2, 2, 8, 8))
    with tg.train_glue("torch"):
        d, p = tg.depth_head(raw.clone().requires_grad_(), 0, ref.MIN_Z, ref.MAX_Z)
    assert type(d.grad_fn).__name__ != "DepthHeadBackward" and not p.requires_grad
    with tg.train_glue("hip"), torch.no_grad():
        d2, p2 = tg.depth_head(raw, 0, ref.MIN_Z, ref.MAX_Z)
    d64, bound = ref.depth_bound(raw, 0)
    assert ref.check("no_grad depth", d2, d64, bound) <= 1.0 and ref.same_bits(p2, ref.pred_img_host(d2))
